"""Generate the golden vectors of the sequential recommenders (FPMC, TransRec) by RUNNING THE REFERENCE:

    python tests/golden/make_golden_seq.py all

Same rules as make_golden.py, whose helpers are reused: every section runs in a fresh process (the reference's
sampler stream is process-global), only data is written.  The fixture set is ``tiny_dataset`` without user 63's
test rows: that user has no training history, and the reference's FPMC / TransRec raise ``KeyError: 63`` when
they evaluate it (FPMC.py:147, TransRec.py:158).
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

SEQ_DIR = os.path.join(G.SCRATCH, "tiny_seq")
PRED_USERS = np.int32([0, 3, 9, 62])


def make_dataset():
    d = np.load(os.path.join(HERE, "tiny_dataset.npz"))
    tr, te = d["train"], d["test"]
    te = te[te[:, 0] != 63]
    os.makedirs(SEQ_DIR, exist_ok=True)
    for name, arr in (("train", tr), ("test", te)):
        with open(os.path.join(SEQ_DIR, "tiny_seq." + name), "w") as f:
            for u, i, t in arr:
                f.write(f"{int(u)}\t{int(i)}\t1.0\t{int(t)}\n")
    np.savez_compressed(os.path.join(HERE, "tiny_seq_dataset.npz"), train=tr, test=te,
                        num_users=int(d["num_users"]), num_items=int(d["num_items"]))
    print("seq dataset:", len(tr), "train /", len(te), "test")


def _loss_recorder(M):
    bpr, l2 = [], []
    ob, ol = M.bpr_loss, M.l2_loss

    def rb(a, b):
        r = ob(a, b); bpr.append(float(r.sum())); return r

    def rl(*w):
        r = ol(*w); l2.append(float(r)); return r
    M.bpr_loss, M.l2_loss = rb, rl
    return bpr, l2


def _fit(model, M, name, tables0, tables1):
    out = {k: v.detach().numpy().copy() for k, v in tables0().items()}
    bpr, l2 = _loss_recorder(M)
    reports = G._record_reports(model)
    best = model.fit()
    out.update({k: v.detach().numpy().copy() for k, v in tables1().items()})
    out.update(bpr_sum=np.float32(bpr), l2=np.float32(l2), reports=np.stack(reports),
               names=np.array(model.evaluator.metrics_list), best=np.array(list(best.values()), np.float32),
               pred_users=PRED_USERS, pred=model.predict(list(PRED_USERS)))
    np.savez_compressed(os.path.join(HERE, f"golden_{name}.npz"), **out)
    print(f"{name}: steps", len(bpr), "first/last bpr", bpr[0], bpr[-1], "NDCG@10", dict(best.items())["NDCG@10"])


def _cfg(name):
    return G._run_config(recommender=name, data_dir=SEQ_DIR)


def make_fpmc():
    G._install()
    import torch
    torch.set_num_threads(1)
    import skrec.recommender.FPMC as M
    G._seed_all()
    model = M.FPMC(_cfg("FPMC"), dict(lr=1e-3, reg=1e-3, embed_size=64, batch_size=256, epochs=3))
    f = model.fpmc

    def tables(sfx):
        return lambda: {"UI" + sfx: f.UI_embeddings.weight, "IU" + sfx: f.IU_embeddings.weight,
                        "IL" + sfx: f.IL_embeddings.weight, "LI" + sfx: f.LI_embeddings.weight}
    _fit(model, M, "fpmc", tables("0"), tables("1"))


def make_transrec():
    G._install()
    import torch
    torch.set_num_threads(1)
    import skrec.recommender.TransRec as M
    G._seed_all()
    model = M.TransRec(_cfg("TransRec"), dict(lr=1e-3, reg=1e-3, embed_size=64, batch_size=256, epochs=3))
    t = model.transrec

    def tables(sfx):
        return lambda: {"U" + sfx: t.user_embeddings.weight, "V" + sfx: t.item_embeddings.weight,
                        "b" + sfx: t.item_biases.weight, "T" + sfx: t.global_transition}
    _fit(model, M, "transrec", tables("0"), tables("1"))


SECTIONS = {"dataset": make_dataset, "fpmc": make_fpmc, "transrec": make_transrec}

if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "all"
    if what == "all":
        for s in SECTIONS:
            subprocess.run([sys.executable, os.path.abspath(__file__), s], check=True)
    else:
        SECTIONS[what]()
