"""Timing of the kNN kernel at bench scale on one GPU:

    python tools/knn_timing.py [--items 100000 --img_dim 4096 --txt_dim 384 --k 10 --repeats 3 --chunk 4096
                                --out profiles/knn_timing.json]

Data: seeded random item features, as tools/bm3_timing.py draws them.  Reported per modality, as one JSON line, medians of
``--repeats`` repeats after one warm-up call: seconds of skr_knn_topk (both launches), its fraction of the arithmetic floor
``2 I^2 F / 157.3 TF`` of the exact-fp32 matrix pipe, and beside it, in the same session, the reference's construction written
with torch-ROCm ops in row chunks (what a user of the reference can run at this size, the dense [I, I] matrix being 40 GB):
``X / |X|`` once, then per chunk of ``--chunk`` rows ``torch.mm`` + ``torch.topk`` -- restated here from
recommender/FREEDOM.py:126-129.  ``same_sets`` is the fraction of rows whose neighbour sets agree between the two (random
features have near-ties: the two sum in different orders).  Every figure comes from one session."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "scikit-recommender_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from skrec import _hip  # noqa: E402
from skrec.utils.item_graph import knn_topk  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12


def _time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def _median(fn, repeats):
    fn()                                   # warm-up
    runs = [_time(fn) for _ in range(repeats)]
    return float(np.median([t for t, _ in runs])), runs[-1][1]


def torch_chunked(X, k, chunk):
    xn = X.div(torch.norm(X, p=2, dim=-1, keepdim=True))
    out = torch.empty((X.shape[0], k), dtype=torch.int64, device=X.device)
    for r0 in range(0, X.shape[0], chunk):
        sim = torch.mm(xn[r0:r0 + chunk], xn.T)
        out[r0:r0 + chunk] = torch.topk(sim, k, dim=-1)[1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--img_dim", type=int, default=4096)
    ap.add_argument("--txt_dim", type=int, default=384)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    args = ap.parse_args()
    dev = _hip.require_gpu()
    g = torch.Generator(device=dev)
    g.manual_seed(2021)
    res = dict(items=args.items, k=args.k, repeats=args.repeats, chunk=args.chunk, device=torch.cuda.get_device_name(0), runs=[])
    for key, F in (("img", args.img_dim), ("txt", args.txt_dim)):
        if not F:
            continue
        X = torch.randn((args.items, F), generator=g, device=dev)
        floor = 2.0 * args.items * args.items * F / FP32_MATRIX_PEAK
        ours_s, ids = _median(lambda: knn_topk(X, args.k), args.repeats)
        run = dict(modality=key, feat_dim=F, knn_s=round(ours_s, 4), floor_s=round(floor, 4), fraction_of_floor=round(floor / ours_s, 4),
                   tflops=round(2.0 * args.items * args.items * F / ours_s / 1e12, 2))
        print(json.dumps(run), flush=True)
        try:
            torch_s, tids = _median(lambda: torch_chunked(X, args.k, args.chunk), args.repeats)
            same = (torch.sort(ids.long(), dim=1)[0] == torch.sort(tids, dim=1)[0]).all(dim=1).float().mean()
            run.update(torch_chunked_s=round(torch_s, 4), speedup_vs_torch=round(torch_s / ours_s, 3), same_sets=round(float(same), 6))
        except RuntimeError as e:          # e.g. out of memory
            run["torch_error"] = str(e)[:200]
        print(json.dumps(run), flush=True)
        res["runs"].append(run)
        del X
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
