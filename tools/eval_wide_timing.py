"""Timing of the fused top-K evaluator at rows of 64 / 128 / 192 / 256 floats on one GPU:

    python tools/eval_wide_timing.py [--users 65536 --items 100000 --inter 3276800 --eval_users 65536 --top_k 20
                                      --repeats 3 --parent_lib PATH/libskrec_hip.so --out profiles/eval_wide_timing.json]

Data: bench.synth_dataset's train rows (imported, not copied; bench.py's catalogue and its 50 interactions per user, over the
evaluated users only, so that a leg does not spend its time building rows nobody ranks) as the mask, N(0, 0.1) factor tables
and an item bias.  Without
--leg this is a driver: every leg runs in a child process of its own under its own time limit (--leg_timeout), the driver
stops at the first leg that fails, and one JSON document is written.  Legs, medians of --repeats after one warm-up call:

* ``w<width>_<mode>`` for the four widths and the two split arithmetics: one skr_eval_fused_topk call over the evaluated
  users, and beside it the dense route the evaluator took for widths above 64 before the wide kernels existed --
  skr_score_matrix + skr_mask_train + skr_eval_scores over chunks of 256 MB of scores, as RankingEvaluator chunks them.
* ``parent64`` (with --parent_lib: the library built from the parent commit): the 64-column f16x2 call of this library and of
  the parent's, loaded side by side and ALTERNATED call by call in one process.

The driver adds ``ratio``: t(width) / (C * t(64)) per mode, C = width / 64 (the matrix work and the item stream grow with C,
the candidate path does not), and ``fused_faster_than_dense`` per leg."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "scikit-recommender_amd"), os.path.join(REPO, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

WIDTHS = (64, 128, 192, 256)
MODES = ("f16x2", "bf16x3")
SCORE_CHUNK_BYTES = 256 << 20


def _spread(v):
    v = sorted(float(x) for x in v)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4))


def _time(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _setup(args, width):
    import torch
    from bench import synth_dataset
    from skrec import _hip
    dev = _hip.require_gpu()
    ds = synth_dataset(args.users, args.items, args.inter, 2021, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    U = torch.randn((args.users, width), generator=g, device=dev) * 0.1
    V = torch.randn((args.items, width), generator=g, device=dev) * 0.1
    bias = torch.randn(args.items, generator=g, device=dev) * 0.01
    users = torch.arange(min(args.users, args.eval_users), dtype=torch.int32, device=dev)
    return torch, _hip, dev, ds, U, V, bias, users


def _fused_call(L, _hip, U, users, V, bias, ds, K, width, ids, sc, work):
    return L.skr_eval_fused_topk(_hip.ptr(U), _hip.ptr(users), users.numel(), _hip.ptr(V), _hip.ptr(bias), V.shape[0], width,
                                 _hip.ptr(ds["rowptr"]), _hip.ptr(ds["items"]), K, _hip.ptr(ids), _hip.ptr(sc), _hip.ptr(work),
                                 work.numel(), _hip.stream())


def leg_width(args, width, mode):
    os.environ["SKR_FUSED_MODE"] = mode
    torch, _hip, dev, ds, U, V, bias, users = _setup(args, width)
    L, K, n, nI = _hip.lib(), args.top_k, users.numel(), args.items
    ids = torch.empty((n, K), dtype=torch.int32, device=dev)
    sc = torch.empty((n, K), dtype=torch.float32, device=dev)
    work = torch.empty(int(L.skr_eval_fused_workspace(n, K)), dtype=torch.uint8, device=dev)

    def fused():
        _hip.check(_fused_call(L, _hip, U, users, V, bias, ds, K, width, ids, sc, work))
    chunk = max(1, min(n, SCORE_CHUNK_BYTES // (4 * nI)))
    d_sc = torch.empty((chunk, nI), dtype=torch.float32, device=dev)
    ids_d = torch.empty((n, K), dtype=torch.int32, device=dev)

    def dense():
        st = _hip.stream()
        for s in range(0, n, chunk):
            b = min(chunk, n - s)
            du = users[s:s + b]
            _hip.check(L.skr_score_matrix(_hip.ptr(U), _hip.ptr(du), b, _hip.ptr(V), _hip.ptr(bias), nI, width, _hip.ptr(d_sc), nI, st))
            _hip.check(L.skr_mask_train(_hip.ptr(d_sc), b, nI, nI, _hip.ptr(du), _hip.ptr(ds["rowptr"]), _hip.ptr(ds["items"]), st))
            _hip.check(L.skr_eval_scores(_hip.ptr(d_sc), b, nI, nI, None, None, None, 0, K, None, _hip.ptr(ids_d[s:s + b]), None, st))
    res = {}
    for name, fn in (("fused", fused), ("dense", dense)):
        fn()
        res[f"{name}_ms"] = _spread([_time(fn, torch) for _ in range(args.repeats)])
    rej = C.c_int32(-1)
    fused()
    _hip.check(L.skr_eval_fused_rejected(C.byref(rej), _hip.stream()))
    res["rejected"] = rej.value
    res["ids_equal_dense_share"] = round(float((ids == ids_d).float().mean()), 5)
    res["users_per_s_fused"] = round(n / (res["fused_ms"]["median"] * 1e-3))
    res["users_per_s_dense"] = round(n / (res["dense_ms"]["median"] * 1e-3))
    return res


def leg_parent64(args):
    os.environ["SKR_FUSED_MODE"] = "f16x2"
    torch, _hip, dev, ds, U, V, bias, users = _setup(args, 64)
    K, n = args.top_k, users.numel()
    libs = {"this": _hip.lib()}
    P = C.CDLL(args.parent_lib)
    res_t, arg_t = _hip.SIGNATURES["skr_eval_fused_topk"]
    P.skr_eval_fused_topk.restype, P.skr_eval_fused_topk.argtypes = res_t, arg_t
    libs["parent"] = P
    ids = {k: torch.empty((n, K), dtype=torch.int32, device=dev) for k in libs}
    sc = torch.empty((n, K), dtype=torch.float32, device=dev)
    work = torch.empty(int(libs["this"].skr_eval_fused_workspace(n, K)), dtype=torch.uint8, device=dev)
    times = {k: [] for k in libs}
    for k in libs:
        _hip.check(_fused_call(libs[k], _hip, U, users, V, bias, ds, K, 64, ids[k], sc, work))
    for _ in range(max(args.repeats, 5)):
        for k in libs:                                # alternated call by call
            times[k].append(_time(lambda: _hip.check(_fused_call(libs[k], _hip, U, users, V, bias, ds, K, 64, ids[k], sc, work)), torch))
    return dict(this_ms=_spread(times["this"]), parent_ms=_spread(times["parent"]),
                ids_equal=bool(torch.equal(ids["this"], ids["parent"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--items", type=int, default=100_000)
    ap.add_argument("--inter", type=int, default=3_276_800)
    ap.add_argument("--eval_users", type=int, default=65536)
    ap.add_argument("--top_k", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent_lib", default=None)
    ap.add_argument("--leg", default=None)
    ap.add_argument("--leg_timeout", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_wide_timing.json"))
    args = ap.parse_args()
    if args.leg:
        if args.leg == "parent64":
            print(json.dumps(leg_parent64(args)))
        else:
            w, mode = args.leg.split("_")
            print(json.dumps(leg_width(args, int(w[1:]), mode)))
        return 0
    legs = [f"w{w}_{m}" for m in MODES for w in WIDTHS] + (["parent64"] if args.parent_lib else [])
    res = dict(users=args.users, items=args.items, eval_users=min(args.users, args.eval_users), top_k=args.top_k,
               repeats=args.repeats, legs={})
    for leg in legs:
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg]
        for k in ("users", "items", "inter", "eval_users", "top_k", "repeats"):
            cmd += [f"--{k}", str(getattr(args, k))]
        if args.parent_lib:
            cmd += ["--parent_lib", args.parent_lib]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if p.returncode != 0:                         # nothing more is started on the GPU behind a leg that failed
            res["failed"] = dict(leg=leg, returncode=p.returncode, stderr=p.stderr[-2000:])
            break
        res["legs"][leg] = json.loads(p.stdout.strip().splitlines()[-1])
        print(leg, json.dumps(res["legs"][leg]), flush=True)
    ratio = {}
    for m in MODES:
        base = res["legs"].get(f"w64_{m}")
        for w in WIDTHS[1:]:
            cur = res["legs"].get(f"w{w}_{m}")
            if base and cur:
                ratio[f"w{w}_{m}"] = round(cur["fused_ms"]["median"] / ((w // 64) * base["fused_ms"]["median"]), 3)
    res["ratio"] = ratio
    res["fused_faster_than_dense"] = {k: v["fused_ms"]["median"] < v["dense_ms"]["median"] for k, v in res["legs"].items()
                                      if "fused_ms" in v}
    try:
        import torch
        res["device"] = torch.cuda.get_device_name(0)
    except Exception:
        pass
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 1 if "failed" in res else 0


if __name__ == "__main__":
    sys.exit(main())
