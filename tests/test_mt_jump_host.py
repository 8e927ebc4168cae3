"""CPU suite: the host half of the jump-ahead word generator (skr_mt_jump_host, csrc/mt_jump.hip) lands where the stream gets
word by word -- several seeds, start positions inside a block, and jumps of g * J words (J = 624 * 2^k, the device's piece
lengths) as well as the head length and odd counts."""
import ctypes as C

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the package on sys.path)
from oracle import oracle as O

HEAD = 33 * 624


def _jump(words, pos, n):
    from skrec import _hip
    out = np.zeros(624, np.uint32)
    p = C.c_int(-1)
    w = np.ascontiguousarray(words, np.uint32)
    _hip.check(_hip.lib().skr_mt_jump_host(w.ctypes.data, int(pos), int(n), out.ctypes.data, C.byref(p)))
    return out, p.value


@pytest.mark.parametrize("seed,skip,n", [
    (2020, 0, 0), (2020, 0, 624), (2020, 5, 619), (2020, 5, 620), (7, 100, 1),
    (7, 100, HEAD - 100), (99, 623, HEAD + 3 * 4992 - 623), (99, 0, 5 * 9984), (12345, 311, 2 * 624 * 64 + 17),
    (2020, 1000, 3 * 19968), (31337, 624, 7 * 2496), (5, 400, 100_003),
])
def test_jump_lands_on_the_stream(seed, skip, n):
    ref = O.Sampler(seed)
    for _ in range(skip):
        ref.next_u32()
    w0, p0 = ref.get_state()
    got, gp = _jump(w0, p0, n)
    for _ in range(n):
        ref.next_u32()
    wr, pr = ref.get_state()
    if pr != 624 or p0 + n <= 624:      # same block: the state itself, every bit of it (the first word's low 31 bits too)
        assert gp == pr and np.array_equal(got, wr)
    else:                                # the stream stands at a block's end; the jump gives the next block at 0
        assert gp == 0
    jumped = O.Sampler(1)
    jumped.set_state(got, gp)
    assert [jumped.next_u32() for _ in range(1300)] == [ref.next_u32() for _ in range(1300)]


def test_jump_rejects_bad_arguments():
    from skrec import _hip
    L = _hip.lib()
    w = np.zeros(624, np.uint32)
    p = C.c_int(0)
    assert L.skr_mt_jump_host(w.ctypes.data, 625, 1, w.ctypes.data, C.byref(p)) == -1
    assert L.skr_mt_jump_host(w.ctypes.data, 0, -1, w.ctypes.data, C.byref(p)) == -1
    assert L.skr_mt_jump_host(None, 0, 1, w.ctypes.data, C.byref(p)) == -1
