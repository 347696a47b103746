// TEST INFRASTRUCTURE ONLY: the scalar device functions of stgcn_device.hip.h, compiled for the host against the emulation shim exactly as
// the emulated library compiles them, behind a C entry each (tests/test_emu_conditioning.py sweeps them against float64).
#include "stgcn_device.hip.h"

extern "C" void probe_tanh(const float* x, float* t, int n) {
    for (int i = 0; i < n; ++i) t[i] = stgcn::tanh_f(x[i]);
}

extern "C" void probe_gate_bwd(const float* dh, const float* u, const float* s, int act, float* du, float* dq, int n) {
    for (int i = 0; i < n; ++i) stgcn::gate_bwd(dh[i], u[i], s[i], act, du[i], dq[i]);
}

extern "C" void probe_relu(const float* x, float* y, int n) {
    for (int i = 0; i < n; ++i) y[i] = stgcn::relu_f(x[i]);
}
