"""Gradient clipping by global norm inside the optimizer step (max_grad_norm) on the emulator: the norm kernel through the C ABI, the three
optimizers against clip_grad_norm_ + torch / the reference's Lion, max_grad_norm = inf against the unclipped path, the two norm producers
(stgcn_grad_norm, the flush epilogue) on a model, and the data-parallel split.  The cases are those of tests/test_gpu_grad_clip.py
(tests/grad_clip_util.py)."""
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import grad_clip_util as U
from tests.emu_util import bind_emulator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cpu"


@pytest.mark.parametrize("case", sorted(U.norm_tables()))
def test_norm_kernel(case):
    """|total - float64 norm| <= 2^-23 norm (squares and sums are fp64: the one fp32 rounding is the stored total), coef is the fp32
    expression on the returned total exactly, a second pass leaves bit-identical words, one NaN element gives a NaN total."""
    U.check_norm_case(bind_emulator(), DEV, case)


def test_c_abi_refuses_small_state_and_bad_max_norm():
    U.check_refusals(bind_emulator(), DEV)


@pytest.mark.parametrize("name", U.ALL_KINDS)
def test_optimizer_trajectory_matches_clip_grad_norm_and_reference(name):
    bind_emulator()
    U.check_optimizer_trajectory(name, DEV)


def test_two_groups_share_one_norm():
    bind_emulator()
    U.check_two_groups_share_one_norm(DEV)


@pytest.mark.parametrize("name", U.ALL_KINDS)
def test_infinite_max_norm_is_bitwise_the_unclipped_path(name):
    bind_emulator()
    U.check_inf_is_bitwise_unclipped(name, DEV)


def test_two_producers_agree():
    bind_emulator()
    U.check_two_producers_agree(DEV)


def test_two_producers_agree_big_table_forms():
    """the same in a fresh process with reduce_kernel's dvec and 4-slice job forms forced on the small model (STGCN_REDUCE_BIG)"""
    env = dict(os.environ, STGCN_REDUCE_BIG="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_emu_grad_clip.py", "-x", "-q", "-p", "no:cacheprovider", "-k",
                        "test_two_producers_agree and not big_table"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout, r.stdout[-2000:]


def test_make_optimizer_and_state_dict_carry_max_grad_norm():
    from stgcn_amd.train import make_optimizer
    m = torch.nn.Linear(3, 2)
    for name in U.ALL_KINDS:
        assert make_optimizer(m, name=name).param_groups[0]["max_grad_norm"] is None
        o = make_optimizer(m, name=name, max_grad_norm=2.5)
        sd = o.state_dict()
        assert sd["param_groups"][0]["max_grad_norm"] == 2.5
        o2 = make_optimizer(m, name=name)
        o2.load_state_dict(sd)
        assert o2._max_grad_norm() == 2.5
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="max_grad_norm"):
                make_optimizer(m, name=name, max_grad_norm=bad)


# ---- data parallel: 2 gloo ranks x half the batch, clipping the all-reduced mean gradient == one process on the whole batch ------------------
MAX_NORM = 0.05        # well below the gradient norm of these steps: both clip


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from stgcn_amd.train import FlatGradAllReduce, GradArena, fused_train_step, init_distributed, make_optimizer, train_step
    from tests.test_dp_gloo import _data, _make
    torch.set_num_threads(1)
    init_distributed("gloo")
    model = _make()
    x, y = _data()
    bl = x.shape[0] // world
    xs, ys = x[rank * bl:(rank + 1) * bl], y[rank * bl:(rank + 1) * bl]
    opt = make_optimizer(model, max_grad_norm=MAX_NORM)
    train_step(model, opt, xs, ys, FlatGradAllReduce(list(model.parameters()), world))
    norms = [float(opt.last_grad_norm.item())]
    arena = GradArena([p for p in model.parameters() if p.grad is not None])
    fused_train_step(model, opt, xs, ys, arena, world=world, all_reduce=dist.all_reduce)      # (what GraphedTrainStep captures for world > 1)
    norms.append(float(opt.last_grad_norm.item()))
    if rank == 0:
        torch.save({"norms": norms, "params": {k: v.clone() for k, v in model.state_dict().items()}}, out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_clip_the_mean_gradient_like_one_big_batch(tmp_path):
    """the pattern of tests/test_dp_gloo.py with clipping on: the norm is that of the all-reduced mean gradient, measured after the
    collective, so parameters (that file's bar, 2e-6) and last_grad_norm (1e-5 relative, its gradient bar) equal the single-process run."""
    from stgcn_amd.train import make_optimizer, train_step
    from tests.test_dp_gloo import _data, _make
    out = str(tmp_path / "r0.pt")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = torch.load(out)
    model = _make()
    x, y = _data()
    opt = make_optimizer(model, max_grad_norm=MAX_NORM)
    for k in range(2):
        train_step(model, opt, x, y, None)
        ref = float(opt.last_grad_norm.item())
        assert ref > 2 * MAX_NORM and float(opt.last_clip_coef.item()) < 0.5
        assert abs(got["norms"][k] - ref) <= 1e-5 * ref, (k, got["norms"][k], ref)
    for k, v in model.state_dict().items():
        assert (got["params"][k] - v).abs().max() <= 2e-6, k
