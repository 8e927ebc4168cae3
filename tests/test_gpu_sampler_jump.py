"""GPU suite: the jump-ahead word generator and the parallel slab resolve (sampler.hip 2e / 2d) against the one-workgroup
generator and the one-lane walk they replace (SKR_MT_JUMP=0, SKR_SLAB_WALK=1): the same words, negatives, stream state,
word count and hand-over report, bit for bit."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

HEAD = 33 * 624


def _words(s, n):
    import torch
    from skrec import _hip
    out = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    _hip.check(_hip.lib().skr_sampler_words(s.handle, int(n), _hip.ptr(out), _hip.stream()))
    return out[:n].cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("skip", [0, 1, 300, 623, 624])
def test_jump_generator_words_and_state(skip, monkeypatch):
    """calls shorter than a block, just below the jump threshold (one workgroup), and of 3, 9, 22, 69 and 127 pieces after
    the head (the most a call takes), starting anywhere in a block; the first calls also against the reference stream"""
    from skrec.utils.py.random import DeviceSampler
    ref = O.Sampler(2020)
    for _ in range(skip):
        ref.next_u32()
    w0, p0 = ref.get_state()
    lens = [5, 623, 2 * HEAD - 1, 2 * HEAD + 700, 100_000, 235_000, 700_000, 127 * 19968 + HEAD - 2 * 624, 7]
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("SKR_MT_JUMP", mode)
        s = DeviceSampler(1)
        s.set_state(w0, p0)
        outs, states = [], []
        for n in lens:
            outs.append(_words(s, n))
            states.append(s.get_state())
        got[mode] = (outs, states, s.draws)
    for k, n in enumerate(lens):
        assert np.array_equal(got["1"][0][k], got["0"][0][k]), n
        assert np.array_equal(got["1"][1][k][0], got["0"][1][k][0]) and got["1"][1][k][1] == got["0"][1][k][1], n
    assert got["1"][2] == got["0"][2] == sum(lens)
    for k in range(5):
        assert np.array_equal(got["1"][0][k], np.array([ref.next_u32() for _ in range(lens[k])], np.uint32)), lens[k]


def _slab_stats(s):
    import ctypes as C
    from skrec import _hip
    info = (C.c_int64 * 2)()
    _hip.check(_hip.lib().skr_sampler_slab_stats(s.handle, info))
    return int(info[0]), int(info[1])


def _csr_from_lens(rng, lens, num_items):
    rowptr = np.zeros(len(lens) + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    pos = np.concatenate([np.sort(rng.choice(num_items, l, replace=False)) for l in lens if l > 0] + [np.zeros(0, np.int64)])
    return rowptr, pos.astype(np.int32)


def _case(name):
    rng = np.random.default_rng({"uniform": 11, "empties": 12, "burst": 13, "dense": 14, "nn2": 15, "tiny_rows": 16}[name])
    nn = 1
    if name == "uniform":
        I, lens = 4000, rng.integers(20, 120, 6000)
    elif name == "empties":       # owners more than SLAB_BND users below the highest candidate: hand-over
        I, lens = 50_000, np.where(rng.random(400_000) < 0.1, rng.integers(1, 6, 400_000), 0)
    elif name == "burst":         # more rejections inside a slab than the window allows: hand-over mid-stream
        I, lens = 3200, np.concatenate([np.full(45_000, 2), np.full(100, 200), np.full(45_000, 2)])
    elif name == "dense":         # blocks of long rows: more events than the resolver holds -> hand-over in the first slab
        I, lens = 1000, np.concatenate([np.full(30_000, 3), np.full(4000, 40), np.full(30_000, 3), np.full(3000, 50)])
    elif name == "tiny_rows":     # one-slot rows among long ones: hand-over in the first slab as well
        I, lens = 800, np.where(rng.random(200_000) < 0.97, 1, 45)
    else:
        I, nn, lens = 2000, 2, rng.integers(0, 90, 3000)
    rowptr, pos = _csr_from_lens(rng, lens, I)
    return I, nn, rowptr, pos


@pytest.mark.parametrize("case", ["uniform", "empties", "burst", "dense", "tiny_rows", "nn2"])
def test_parallel_resolve_and_jump_match_walk(case, monkeypatch):
    """every combination of generator and resolver, and the rounds capped at 1 so that the walk takes over from unsettled
    rounds: the same negatives, hand-over report, state and word count.  Where the slabs finish the stream (uniform, nn2: about
    2 % rejections, slabs of 8 192 draws) the slabs take up to a dozen rounds, and a cap of one hands them to the walk"""
    from gpu_utils import ExactSampler
    I, nn, rowptr, pos = _case(case)
    monkeypatch.setenv("SKR_EXACT_PATH", "slab")
    runs, stats = {}, {}
    for jump, walk, cap in (("0", "1", "32"), ("1", "0", "32"), ("0", "0", "32"), ("1", "1", "32"), ("1", "0", "1")):
        monkeypatch.setenv("SKR_MT_JUMP", jump)
        monkeypatch.setenv("SKR_SLAB_WALK", walk)
        monkeypatch.setenv("SKR_SLAB_ROUNDS", cap)
        gpu = ExactSampler(2020)
        outs, st = [], []
        for _ in range(2):
            outs.append((gpu.epoch(I, rowptr, pos, nn), gpu.s.last_epoch()))
            st.append(_slab_stats(gpu.s))
        runs[(jump, walk, cap)] = (outs, gpu.s.get_state(), gpu.s.draws)
        stats[(jump, walk, cap)] = st
    assert all(st == (0, 0) for st in stats[("0", "1", "32")] + stats[("1", "1", "32")])
    rounds = max(r for r, _ in stats[("1", "0", "32")])
    if case in ("uniform", "nn2"):
        assert rounds > 1, stats
    if rounds > 1:                       # a slab that needed a second round cannot settle under a cap of one
        assert sum(w for _, w in stats[("1", "0", "1")]) > 0, stats
    base = runs[("0", "1", "32")]
    for key, r in runs.items():
        for (a, ia), (b, ib) in zip(r[0], base[0]):
            assert np.array_equal(a, b), key
            assert ia == ib, (key, ia, ib)
        assert np.array_equal(r[1][0], base[1][0]) and r[1][1] == base[1][1] and r[2] == base[2], key
    ref = O.Sampler(2020)
    want = ref.sample_epoch(I, rowptr, pos, nn).reshape(-1)
    assert np.array_equal(base[0][0][0], want)


@pytest.mark.timeout(900)
def test_full_size_slice_and_epoch(monkeypatch):
    """bench.py's data set (1 M users / 100 k items): the timed slice's size (200 batches of 1 024) and a whole epoch, new
    generator and resolve against the old ones: identical negatives, stream state, word count and report"""
    import torch
    import bench
    from skrec.utils.py.random import DeviceSampler
    ds = bench.synth_dataset(1_000_000, 100_000, 50_000_000, 20260101, torch.device("cuda", 0))
    rowptr, items = ds["rowptr"], ds["items"]
    n_sl = int(torch.searchsorted(rowptr, torch.tensor(200 * 1024, device=rowptr.device))) + 1
    slices = [(n_sl, rowptr[:n_sl + 1].contiguous(), items), (1_000_000, rowptr, items)]
    res = {}
    for jump, walk in (("1", "0"), ("0", "1")):
        monkeypatch.setenv("SKR_MT_JUMP", jump)
        monkeypatch.setenv("SKR_SLAB_WALK", walk)
        s = DeviceSampler(2020)
        outs = []
        for nU, rp, it in slices + slices[:1]:
            nnz = int(rp[-1])
            neg = torch.empty(nnz, dtype=torch.int32, device="cuda")
            s.sample_epoch_exact(100_000, nU, rp, it, nnz, 1, neg)
            w, p = s.get_state()
            outs.append((neg.cpu().numpy(), w, p, s.draws, s.last_epoch()))
        res[jump] = outs
    for a, b in zip(res["1"], res["0"]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
