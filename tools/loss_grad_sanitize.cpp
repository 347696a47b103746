// The stand-alone loss launch (stgcn_loss_grad, every kind and every label mode) under AddressSanitizer + UndefinedBehaviorSanitizer on
// the CPU: the library's own sources compiled by the host clang against the emulation shim (tests/emu), linked with this main -- a
// program of its own, nothing is loaded into python.  Every buffer is a heap allocation of exactly the size the call may touch, so an
// access outside of it is reported.  The cases are those of tests/test_emu_loss_kinds.py's stand-alone part.
//
// (-O0: about a minute; the instrumented single translation unit of the whole library takes more than half an hour at -O1.)
//
//   clang++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -O0 -x c++ -I tests/emu \
//       '-DSTGCN_BACKEND_NAME="emu-cpu"' -Wno-unused-value -Wno-vla-cxx-extension stgcn_amd/csrc/stgcn_capi.hip tests/emu/emu_runtime.cpp \
//       tools/loss_grad_sanitize.cpp -o /tmp/loss_grad_sanitize && /tmp/loss_grad_sanitize
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../include/stgcn_hip.h"

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            ++failures;                   \
            printf("FAILED: " __VA_ARGS__); \
            printf("\n");                 \
        }                                 \
    } while (0)

static const float kDelta = 0.5f;

// |off| uniform in [0.05, 0.45] U [0.55, 2.0], random sign: clear of sgn's jump at 0 and of Huber's switch at delta = 0.5
static double offset(std::mt19937& g) {
    std::uniform_real_distribution<double> u(0.0, 0.4 + 1.45);
    const double v = u(g), mag = v < 0.4 ? 0.05 + v : 0.55 + (v - 0.4);
    return (g() & 1) ? mag : -mag;
}

static void reference(int kind, const std::vector<float>& p, const float* y, double scale, double* loss, std::vector<double>& grad) {
    const size_t n = p.size();
    double s = 0;
    grad.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const double d = (double)p[i] - (double)y[i], a = fabs(d), sg = d > 0 ? 1 : d < 0 ? -1 : 0;
        double term, dt;
        if (kind == STGCN_LOSS_MSE) { term = d * d; dt = 2 * d; }
        else if (kind == STGCN_LOSS_MAE) { term = a; dt = sg; }
        else if (a < kDelta) { term = 0.5 * d * d; dt = d; }
        else { term = kDelta * (a - 0.5 * kDelta); dt = kDelta * sg; }
        s += term;
        grad[i] = dt * scale / (double)n;
    }
    *loss = s / (double)n;
}

static void compare(const char* what, int kind, const std::vector<float>& pred, const float* labels, float loss, const std::vector<float>& dpred) {
    double lref, gmax = 0, emax = 0;
    std::vector<double> g;
    reference(kind, pred, labels, 0.5, &lref, g);
    for (size_t i = 0; i < g.size(); ++i) {
        gmax = fmax(gmax, fabs(g[i]));
        emax = fmax(emax, fabs((double)dpred[i] - g[i]));
    }
    CHECK(fabs(loss - lref) <= 1e-6 * fabs(lref), "%s kind %d: loss %g against %g", what, kind, loss, lref);
    CHECK(emax <= 1e-7 * gmax + 1e-12, "%s kind %d: gradient error %g of max %g", what, kind, emax, gmax);
}

int main() {
    std::mt19937 gen(3);
    std::normal_distribution<float> normal(0.f, 1.f);
    const int shapes[3][2] = {{3, 5}, {8, 207}, {32, 325}};
    for (const auto& sh : shapes)
        for (int kind = 0; kind < 3; ++kind) {
            const size_t n = (size_t)sh[0] * sh[1];
            std::vector<float> pred(n), y(n), dpred(n), loss(1);
            for (size_t i = 0; i < n; ++i) {
                pred[i] = normal(gen);
                y[i] = (float)((double)pred[i] - offset(gen));
            }
            y[1] = pred[1];   // pred == target bitwise: a gradient of exactly 0
            int rc = stgcn_loss_grad(kind, kDelta, pred.data(), y.data(), (int64_t)n, 0.5f, loss.data(), dpred.data(), nullptr, 0, nullptr, 0, nullptr);
            CHECK(rc == STGCN_OK, "plain call: rc %d (%s)", rc, stgcn_last_error());
            compare("plain", kind, pred, y.data(), loss[0], dpred);
            CHECK(dpred[1] == 0.f, "kind %d: gradient %g where pred == target", kind, dpred[1]);
            if (kind == STGCN_LOSS_MSE) {   // bitwise the MSE entry
                std::vector<float> d2(n), l2(1);
                rc = stgcn_mse_loss_grad(pred.data(), y.data(), (int64_t)n, 0.5f, l2.data(), d2.data(), nullptr, 0, nullptr);
                CHECK(rc == STGCN_OK && memcmp(l2.data(), loss.data(), sizeof(float)) == 0 && memcmp(d2.data(), dpred.data(), n * sizeof(float)) == 0,
                      "stgcn_mse_loss_grad differs from stgcn_loss_grad(STGCN_LOSS_MSE)");
            }
            // one NaN prediction: NaN loss, NaN gradient there, every other element as before
            std::vector<float> bad(pred), d3(n), l3(1);
            bad[n / 2] = NAN;
            rc = stgcn_loss_grad(kind, kDelta, bad.data(), y.data(), (int64_t)n, 0.5f, l3.data(), d3.data(), nullptr, 0, nullptr, 0, nullptr);
            CHECK(rc == STGCN_OK && isnan(l3[0]) && isnan(d3[n / 2]), "kind %d: a NaN prediction did not stay visible", kind);
            for (size_t i = 0; i < n; ++i)
                if (i != n / 2) CHECK(memcmp(&d3[i], &dpred[i], sizeof(float)) == 0, "kind %d: element %zu moved with a NaN elsewhere", kind, i);
        }
    // index mode and window-table mode: B windows of N labels out of a series of exactly the rows the table names
    {
        const int B = 4, N = 20, rows = 10;
        const int64_t pos = 2, table[8] = {7, 0, 3, 9, 1, 5, 8, 2};
        std::vector<float> series((size_t)rows * N);
        for (auto& v : series) v = normal(gen);
        for (int kind = 0; kind < 3; ++kind)
            for (int mode = 0; mode < 2; ++mode) {
                std::vector<float> gathered((size_t)B * N), pred((size_t)B * N), dpred((size_t)B * N), loss(1);
                for (int b = 0; b < B; ++b) {
                    const int64_t row = mode ? table[pos + b] : pos + b;
                    for (int j = 0; j < N; ++j) {
                        gathered[b * N + j] = series[row * N + j];
                        pred[b * N + j] = (float)((double)gathered[b * N + j] + offset(gen));
                    }
                }
                const int64_t idx[1] = {pos};
                const int rc = stgcn_loss_grad(kind, kDelta, pred.data(), series.data(), (int64_t)B * N, 0.5f, loss.data(), dpred.data(), idx, N,
                                               mode ? table : nullptr, mode ? N : 0, nullptr);
                CHECK(rc == STGCN_OK, "label mode %d: rc %d (%s)", mode, rc, stgcn_last_error());
                compare(mode ? "table" : "index", kind, pred, gathered.data(), loss[0], dpred);
            }
    }
    // refusals, before any launch
    {
        std::vector<float> p(4, 1.f), y(4, 0.f), d(4), l(1);
        CHECK(stgcn_loss_grad(7, 1.f, p.data(), y.data(), 4, 1.f, l.data(), d.data(), nullptr, 0, nullptr, 0, nullptr) == STGCN_ERR_INVALID &&
                  strstr(stgcn_last_error(), "kind 7"), "kind 7 was not refused by name");
        const float deltas[4] = {0.f, -1.f, INFINITY, NAN};
        for (float dl : deltas)
            CHECK(stgcn_loss_grad(STGCN_LOSS_HUBER, dl, p.data(), y.data(), 4, 1.f, l.data(), d.data(), nullptr, 0, nullptr, 0, nullptr) == STGCN_ERR_INVALID &&
                      strstr(stgcn_last_error(), "delta"), "Huber delta %g was not refused", dl);
    }
    printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
