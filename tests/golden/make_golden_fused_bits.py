"""Record the output BITS of skr_eval_fused_topk in its three arithmetics (needs the GPU):

    python tests/golden/make_golden_fused_bits.py [OUTPUT]

writes tests/golden/fused_topk_bits.json (or OUTPUT).  For every case and every SKR_FUSED_MODE it holds a SHA-256 of the returned ids
(int32 bytes), a SHA-256 of the returned scores' bit patterns (uint32 bytes) and the count of skr_eval_fused_rejected; once
per case a SHA-256 of the generated inputs, so that a reader can tell "the inputs differ" (another numpy stream) from "the
kernel differs".  The output of every mode is a pure function of its arithmetic -- the final list is the exact top-K by
key of all scores computed -- so the digests do not depend on when lists were compacted or on the order of the flag list;
they change when the order of the piece products, the split or the summation order changes.  That is the point: run this
ONLY when the arithmetic is meant to change, never to make test_fused_topk_bits_equal_the_recorded_ones pass.

tests/test_gpu_eval.py imports CASES, make_inputs and run_case from here, so the test and the file cannot drift apart.
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "fused_topk_bits.json")
MODES = ("f16x2", "bf16x3", "fp32")

# (B, I, K, bias, mask): each the smallest shape that reaches the named path
CASES = [
    (70, 17, 9, True, True),       # catalogue ends one item into the second 16-item group; second wavefront has 6 users
    (130, 200, 10, True, True),    # three live wavefronts + one that only carries DMA and barriers; ring wraps, bias rows rotate;
                                   # trigger 60 < the 61 items that pass a -inf threshold: one- and two-register selects mid-sweep
    (260, 200, 10, False, True),   # two workgroups, no bias
    (130, 400, 40, True, True),    # trigger rule lands at 150, pulled to 120: two-register final compactions
    (130, 400, 54, False, True),   # trigger 192, lists beyond 128: four-register select and final sort
    (65, 400, 128, True, True),    # top_k at its maximum; trigger cut to cap - step (differs between fp32 and the split kernels)
    (160, 400, 10, False, False),  # 37 user rows scaled by 2^-22: the guard flags them, the row-mapped bf16x3 launch recomputes them
]
SMALL_ROWS_CASE = (160, 400, 10, False, False)
N_SMALL = 37


def make_inputs(case):
    """factors x 0.3, bias x 0.1, random_csr masks from np.random.default_rng(B + I + K), as test_fused_topk_vs_fp64 draws them"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from helpers import random_csr
    B, I, K, with_bias, with_mask = case
    rng = np.random.default_rng(B + I + K)
    nU = B + 17
    Ut = (rng.standard_normal((nU, 64)) * 0.3).astype(np.float32)
    It = (rng.standard_normal((I, 64)) * 0.3).astype(np.float32)
    bias = (rng.standard_normal(I) * 0.1).astype(np.float32) if with_bias else None
    users = rng.permutation(nU)[:B].astype(np.int32)
    max_tr = max(0, min(I - K, 120))
    rowptr, items = random_csr(rng, nU, I, 0, max_tr) if with_mask else (None, np.zeros(0, np.int32))
    if case == SMALL_ROWS_CASE:   # as test_f16x2_guard_hands_rows_it_cannot_vouch_for_to_bf16x3
        Ut[users[rng.permutation(B)[:N_SMALL]]] *= np.float32(2.0 ** -22)
    return Ut, users, It, bias, rowptr, items


def inputs_digest(inp):
    h = hashlib.sha256()
    for a in inp:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_case(inp, K, mode):
    """one call in `mode` -> the three recorded values"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from gpu_utils import fused_topk
    from skrec import _hip
    Ut, users, It, bias, rowptr, items = inp
    old = os.environ.get("SKR_FUSED_MODE")
    os.environ["SKR_FUSED_MODE"] = mode     # read per call
    try:
        ids, sc = fused_topk(Ut, users, It, bias, rowptr, items, K)
        n = ctypes.c_int32(-1)
        _hip.check(_hip.lib().skr_eval_fused_rejected(ctypes.byref(n), _hip.stream()))
    finally:
        if old is None:
            del os.environ["SKR_FUSED_MODE"]
        else:
            os.environ["SKR_FUSED_MODE"] = old
    return {"ids_sha256": hashlib.sha256(np.ascontiguousarray(ids, np.int32).tobytes()).hexdigest(),
            "score_bits_sha256": hashlib.sha256(np.ascontiguousarray(sc, np.float32).view(np.uint32).tobytes()).hexdigest(),
            "rejected": int(n.value)}


def main():
    for p in (REPO, os.path.join(REPO, "scikit-recommender_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    out = {"numpy": np.__version__, "cases": []}
    for case in CASES:
        inp = make_inputs(case)
        rec = {"case": list(case), "inputs_sha256": inputs_digest(inp), "modes": {m: run_case(inp, case[2], m) for m in MODES}}
        if case == SMALL_ROWS_CASE:
            n_rej = rec["modes"]["f16x2"]["rejected"]
            assert N_SMALL <= n_rej < case[0], "guard case: %d rows rejected; choose another seed, not another bound" % n_rej
        out["cases"].append(rec)
        print(rec)
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    assert os.path.getsize(path) < 16 * 1024
    print("wrote", path)


if __name__ == "__main__":
    main()
