"""The host-side trust rule of the LayerNorm hook (tests/hook_trust_util.py) on the CPU emulator: the same cases run under -m gpu in
tests/test_gpu_block_hooks.py."""
import pytest

from tests import hook_trust_util as trust


@pytest.mark.parametrize("tamper", trust.TAMPERS)
def test_producer_runs_its_own_pass_when_the_gradient_is_not_the_consumers(tamper):
    trust.check_tamper("cpu", tamper)


def test_forward_without_backward_leaves_no_offer_behind():
    trust.check_abandoned_forward("cpu")


def test_two_steps_on_the_same_caches():
    trust.check_two_steps("cpu")
