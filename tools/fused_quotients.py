"""How much catch-up a step launch of the fused BPR step does: from the plan words (skrec.recommender.fused.build_fused_meta)
of given id columns, the Adam quotient evaluations per wavefront -- one wavefront per interaction, its five rows one after
the other -- per step index of a k-step block: mean and maximum.  A launch lasts as long as its slowest wavefront, so the
maximum is what tools/fused_lab.py --per-step should follow.

A row named at steps s' < s makes s - s' quotients at s (the gradient update s' and the zero-gradient updates behind it); a
first naming at s makes s (zero-gradient updates from the block's first index) unless the block before did not name the row:
then bpr_fused_pre_kernel made them ahead of time (word field n0 = 7) and the step launch makes none.  Runs the at-rest test
would take (moments decay, no quotient) are counted as if they were not at rest: an upper bound, exact for lively rows.

Host only, no GPU.  The ids are the lab's (uniform users and negatives, positives ~ 1 / (rank + 10)^0.8) or, with --zipf A,
positives ~ 1 / rank^A as the benchmark draws them.
usage: python tools/fused_quotients.py [k] [blocks] [--users N] [--items N] [--batch B] [--zipf A] [--no-pre]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scikit-recommender_amd"))


def quotients(cu, ci, cj, n_blocks, k, bsz, n_users, n_items, pre=True):
    """[n_blocks, k, bsz] int64: quotient evaluations of each interaction's wavefront.  cu / ci / cj: CPU int32 columns,
    step-major; pre: rows the block before did not name are advanced ahead of time (the first block has no block before:
    nothing of it is, as in FusedBlocks)"""
    from skrec.recommender.fused import build_fused_meta
    nfb = ((n_users + n_items) * 64 + n_items + 63) // 64
    rows = n_blocks * k * bsz
    prev_hot = None
    if pre:
        prev_hot = torch.ones((n_blocks, nfb), dtype=torch.bool)
        U, I, J = (c[:rows].view(n_blocks, k * bsz).long() for c in (cu, ci, cj))
        for q in range(1, n_blocks):
            prev_hot[q] = False
            for named in (U[q - 1], n_users + I[q - 1], n_users + J[q - 1], n_users + n_items + (I[q - 1] >> 6),
                          n_users + n_items + (J[q - 1] >> 6)):
                prev_hot[q, named] = True
    meta = build_fused_meta(cu, ci, cj, n_blocks, k, bsz, 0, n_users, n_users + n_items, chunk_blocks=4, prev_hot=prev_hot)[0].long()
    n0f, prev1 = (meta >> 20) & 7, (meta >> 24) & 0x7f                       # [n_blocks, k, 5, bsz]
    step = torch.arange(k).view(1, k, 1, 1)
    per_row = torch.where(prev1 > 0, step - prev1 + 1, torch.where(n0f == 7, torch.zeros_like(step), step))
    return per_row.sum(dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("k", type=int, nargs="?", default=32)
    ap.add_argument("blocks", type=int, nargs="?", default=12)
    ap.add_argument("--users", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--zipf", type=float, default=None)
    ap.add_argument("--no-pre", action="store_true")
    a = ap.parse_args()
    g = torch.Generator().manual_seed(1)
    n = a.k * a.batch * a.blocks
    u = torch.randint(0, a.users, (n,), generator=g, dtype=torch.int32)
    rank = torch.arange(a.items, dtype=torch.float64)
    w = 1.0 / (rank + 1.0) ** a.zipf if a.zipf is not None else 1.0 / (rank + 10.0) ** 0.8
    i = torch.multinomial(w.float(), n, replacement=True, generator=g).int()
    j = torch.randint(0, a.items, (n,), generator=g, dtype=torch.int32)
    q = quotients(u, i, j, a.blocks, a.k, a.batch, a.users, a.items, pre=not a.no_pre)[a.blocks // 2:].numpy()
    mean, mx = q.mean(axis=(0, 2)), q.max(axis=2).mean(axis=0)
    print(f"k={a.k} batch={a.batch} users={a.users} items={a.items} pre={not a.no_pre}: quotients per wavefront, mean {q.mean():.1f}, "
          f"slowest wavefront of a step averaged over the steps {mx.mean():.1f}")
    print("mean per step index 0 .. k-1: " + " ".join(f"{x:.1f}" for x in mean))
    print("slowest wavefront per step index 0 .. k-1: " + " ".join(f"{x:.0f}" for x in mx))


if __name__ == "__main__":
    main()
