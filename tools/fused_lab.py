"""Where the time of skr_bpr_fused_step goes: k launches of a block timed with HIP events, nothing beside them.
SKR_FUSED_DBG (one-wavefront kernel only; results are then wrong, timing only): 1 no catch-up arithmetic, 2 no gradient
atomics, 4 no owner stores, 8 no loss atomics / no store of the loss partials, 32 the partials' store write-through instead of
plain.  The step launches are the deferred-loss form (skr_bpr_fused_step3 / _end3: partials per wavefront, folded by
the end launch); SKR_FUSED_LOSS_DEFER=0 times the form that adds to the loss words itself.  SKR_FUSED_STATS=1: prints the census of the evaluations (skr_fused_census;
its counters slow the launches -- not for timing).
--per-step: an event pair around EACH of the k step launches of a block, and the mean launch time per step index 0 .. k - 1
(the events between the launches cost time themselves: compare builds step by step, not with the figure without the option);
tools/fused_quotients.py counts the catch-up work per step index for the same id distributions.
usage: python tools/fused_lab.py [k] [blocks] [--per-step]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scikit-recommender_amd"))
from skrec import _hip  # noqa: E402

per_step = "--per-step" in sys.argv[1:]
argv = [x for x in sys.argv[1:] if not x.startswith("--")]
k = int(argv[0]) if len(argv) > 0 else 32
n_blocks = int(argv[1]) if len(argv) > 1 else 12
nU, nI, b = 1_000_000, 100_000, 1024
dev = torch.device("cuda:0")
L, st = _hip.lib(), _hip.stream()
n_par = (nU + nI) * 64 + nI
g = torch.Generator(device=dev).manual_seed(1)
flat = torch.randn(n_par, device=dev, generator=g) * 0.01
m1, m2 = torch.zeros_like(flat), torch.zeros_like(flat)
n = k * b * n_blocks
u = torch.randint(0, nU, (n,), device=dev, generator=g, dtype=torch.int32)
w = 1.0 / (torch.arange(nI, device=dev, dtype=torch.float64) + 10.0) ** 0.8
i = torch.multinomial(w.float(), n, replacement=True, generator=g).int()
j = torch.randint(0, nI, (n,), device=dev, generator=g, dtype=torch.int32)
cap = k * 5 * b
work = torch.zeros(9 * cap * 64, device=dev)
meta, sb, sf = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(3))
ns = torch.zeros(1, dtype=torch.int32, device=dev)
nfb = (n_par + 63) // 64
scratch = torch.zeros(28 * nfb // 8 + 1, dtype=torch.int64, device=dev)
loss = torch.zeros(64, device=dev)
defer = os.environ.get("SKR_FUSED_LOSS_DEFER", "1") != "0"
part = torch.empty(int(L.skr_bpr_fused_loss_part_floats(b, k)), device=dev)
ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
t_plan, t_steps, t_end, t_each = [], [], [], []
t = 0
for blk in range(n_blocks):
    o = 4 * blk * k * b
    e = [ev() for _ in range(4)]
    e[0].record()
    _hip.check(L.skr_bpr_fused_plan(u.data_ptr() + o, i.data_ptr() + o, j.data_ptr() + o, b, k, 0, nU, nU + nI, nfb, scratch.data_ptr(),
                                    meta.data_ptr(), sb.data_ptr(), sf.data_ptr(), ns.data_ptr(), st))
    e[1].record()
    rc = 0
    es = [ev() for _ in range(k + 1)] if per_step else None
    for s in range(k):
        if per_step:
            es[s].record()
        q = o + 4 * s * b
        if defer:
            rc |= L.skr_bpr_fused_step3(flat.data_ptr(), m1.data_ptr(), m2.data_ptr(), n_par, work.data_ptr(), cap, u.data_ptr() + q,
                                        i.data_ptr() + q, j.data_ptr() + q, meta.data_ptr() + 20 * s * b, b, 0, nU, nU + nI, 1e-3, 0.9,
                                        0.999, 1e-8, t, k, s, 1e-3, loss.data_ptr(), None, part.data_ptr(), st)
        else:
            rc |= L.skr_bpr_fused_step(flat.data_ptr(), m1.data_ptr(), m2.data_ptr(), n_par, work.data_ptr(), cap, u.data_ptr() + q,
                                       i.data_ptr() + q, j.data_ptr() + q, meta.data_ptr() + 20 * s * b, b, 0, nU, nU + nI, 1e-3, 0.9,
                                       0.999, 1e-8, t, k, s, 1e-3, loss.data_ptr(), st)
    if per_step:
        es[k].record()
    e[2].record()
    if defer:
        rc |= L.skr_bpr_fused_end3(flat.data_ptr(), m1.data_ptr(), m2.data_ptr(), n_par, work.data_ptr(), cap, sb.data_ptr(), sf.data_ptr(),
                                   ns.data_ptr(), 1e-3, 0.9, 0.999, 1e-8, t, k, None, 0, 0, part.data_ptr(), loss.data_ptr(), 0, b, st)
    else:
        rc |= L.skr_bpr_fused_end(flat.data_ptr(), m1.data_ptr(), m2.data_ptr(), n_par, work.data_ptr(), cap, sb.data_ptr(), sf.data_ptr(),
                                  ns.data_ptr(), 1e-3, 0.9, 0.999, 1e-8, t, k, None, 0, 0, st)
    e[3].record()
    _hip.check(rc)
    t += k
    torch.cuda.synchronize()
    t_plan.append(e[0].elapsed_time(e[1])); t_steps.append(e[1].elapsed_time(e[2])); t_end.append(e[2].elapsed_time(e[3]))
    if per_step:
        t_each.append([es[s].elapsed_time(es[s + 1]) for s in range(k)])
h = n_blocks // 2
print(f"k={k} dbg={os.environ.get('SKR_FUSED_DBG', '0')} loss {'deferred (step3 / end3)' if defer else 'added per step (step / end)'}: "
      f"plan {np.mean(t_plan[h:]) * 1e3:.1f} us/block, steps {np.mean(t_steps[h:]) * 1e3 / k:.2f} us/step, end {np.mean(t_end[h:]) * 1e3:.1f} us/block"
      f"  (slots {int(ns)})")
if per_step:
    each = np.mean(np.array(t_each[h:]), axis=0) * 1e3
    print("per-step us, step index 0 .. k-1: " + " ".join(f"{x:.2f}" for x in each))
if os.environ.get("SKR_FUSED_STATS") == "1":
    import ctypes
    cen = (ctypes.c_uint64 * 34)()
    _hip.check(L.skr_fused_census(cen, 34, 0))
    for kn, name in enumerate(("step: rows", "step: bias blocks", "end", "pre")):
        for kd, kind in enumerate(("gradient updates", "zero-gradient runs")):
            c = [int(x) for x in cen[8 * kn + 4 * kd:8 * kn + 4 * kd + 4]]
            if sum(c):
                print(f"census {name:18s} {kind:18s}: at rest {c[0]}, ordinary {c[1]}, general {c[3]}")
    print(f"census end launch: slots paired {int(cen[32])}, one by one {int(cen[33])}")
