"""tests/philox_ref.py against the published known-answer vectors of Philox4x32-10 (Random123's kat_vectors), without the library."""
import numpy as np

from tests import philox_ref as ref

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def test_known_answer_vectors():
    for ctr, key, want in KAT:
        got = ref.philox4x32_10(*ctr, *key)
        assert " ".join(f"{int(w):08x}" for w in got) == want, (ctr, key)
    # ... and vectorised: the three cases in one call
    c = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    k = [np.array([k[1][i] for k in KAT], dtype=np.uint64) for i in range(2)]
    got = np.stack(ref.philox4x32_10(*c, *k), axis=1)
    assert [" ".join(f"{int(w):08x}" for w in row) for row in got] == [k[2] for k in KAT]


def test_keep_mask_layout_threshold_and_scale():
    """Element 4q + j is output j of counter (q, 0, offset lo, offset hi) under key (seed lo, seed hi)."""
    seed, off = (0x299F31D0 << 32) | 0xA4093822, (0x03707344 << 32) | 0x13198A2E
    draws, keep = ref.keep_mask(12, 0.5, seed, off)
    for q in range(3):
        want = ref.philox4x32_10(q, 0, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
        assert [int(d) for d in draws[4 * q:4 * q + 4]] == [int(w) for w in want]
    assert (keep == (draws >= 0x80000000)).all()
    assert ref.threshold(0.0) == 0 and ref.threshold(0.5) == 1 << 31 and ref.threshold(1.0) == 0xFFFFFFFF
    assert ref.threshold(1e-6) == int(float(np.float32(1e-6)) * 2 ** 32) and ref.threshold(0.3) == int(float(np.float32(0.3)) * 2 ** 32)
    assert ref.keep_mask(8, 0.0, 1, 2)[1].all()
    assert ref.keep_scale(0.5) == np.float32(2.0) and ref.keep_scale(0.0) == np.float32(1.0)
    assert ref.keep_scale(0.3).dtype == np.float32
    assert len(ref.keep_mask(6, 0.5, 0, 0)[0]) == 6
