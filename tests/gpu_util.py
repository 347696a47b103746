"""Helpers for the -m gpu tests: run one ST block through the HIP library on cuda:0 and compare every stage with the numpy stage
oracle.  The harness itself is tests/block_util.py, which the emulator tests share."""
from tests import block_util
from tests.block_util import FWD_TOL, GRAD_TOL      # noqa: F401  (tests/head_util.py and the bf16 helpers import the bars from here)


def bind_hip():
    return block_util.bind("cuda:0")


def run_block_case(c_in, channels, Kt, Ks, gct, act, N, B, T, training, gso=None, dev="cuda:0", seed=99, offset=3, pdrop=0.5,
                   debug_stages=True):
    """Returns dict of max errors (absolute for activations, relative-to-max for gradients): block_util.run_block_case on the HIP
    library.  debug_stages=True: the fused kernels' on-chip intermediates (dZ2, dZ1) come from the stage-per-launch kernels, launched in
    front of them; False: the launch sequence of a training step.  Either way the previous setting of the flag is restored on return."""
    bind_hip()
    return block_util.run_block_case(dev, c_in, channels, Kt, Ks, gct, act, N, B, T, training, gso=gso, seed=seed, offset=offset,
                                     pdrop=pdrop, debug_stages=debug_stages, oracle32=False, kink=False)


def assert_errors(err):
    block_util.assert_errors(err)
