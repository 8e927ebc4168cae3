"""CPU suite of the models' shared scaffold (``DeviceRecommender``, skrec/recommender/base.py): the fit loop on a stub with a
scripted evaluator, the order of the constructor's checks for every model on it, and that no model has a loop of its own."""
import importlib

import pytest

from skrec.utils.py import MetricReport

ON_SCAFFOLD = ("CDAE", "MultVAE", "FPMC", "TransRec", "HGN", "LightGCL", "DENS", "SelfCF", "BM3")


def _cls(name):
    return getattr(importlib.import_module(f"skrec.recommender.{name}"), name)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the fit loop
# ---------------------------------------------------------------------------------------------------------------------
class _Lines(object):
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


class _Evaluator(object):
    metrics_str = "NDCG@10     \tRecall@10   "


class _Config(object):
    def __init__(self, epochs, early_stop):
        self.epochs, self.early_stop = epochs, early_stop


def _stub(monkeypatch, epochs, early_stop, ndcg):
    """a model made with ``__new__`` (no data set, no GPU) whose evaluate() hands out the scripted NDCG@10 values"""
    from skrec.parallel import DistContext
    from skrec.recommender.base import DeviceRecommender
    monkeypatch.setenv("SKR_COMPUTE_STREAM", "0")                 # on_compute_stream passes straight through

    class Stub(DeviceRecommender):
        def _build(self):
            raise AssertionError("fit() builds nothing")

        def _make_iterator(self):
            self.iterators += 1
            return "the iterator"

        def train_epoch(self, data_iter, extra=None):
            raise AssertionError("fit() calls train_epoch through the instance's attribute")

        def evaluate(self, test_users=None):
            assert test_users is None
            k = len(self.reports)
            self.reports.append(MetricReport(["NDCG@10", "Recall@10"], [ndcg[k], 0.5 + k]))
            self.order.append(("evaluate", k))
            return self.reports[-1]

    m = Stub.__new__(Stub)
    m.config, m.logger, m.evaluator, m.dist = _Config(epochs, early_stop), _Lines(), _Evaluator(), DistContext(0, 1)
    m.iterators, m.reports, m.order = 0, [], []

    def train_epoch(*args, **kwargs):                             # the one-argument wrapper the GPU tests put in its place
        assert args == ("the iterator",) and not kwargs
        m.order.append(("train", len(m.reports)))
    m.train_epoch = train_epoch
    return m


def _line(head, report):
    return head.ljust(12) + "\t" + report.values_str


def test_fit_stops_early_and_returns_the_best(monkeypatch):
    # 0.1 is the first best, 0.3 improves; 0.2 and a second 0.3 (not better: <=) are two evaluations without improvement
    m = _stub(monkeypatch, epochs=10, early_stop=2, ndcg=[0.1, 0.3, 0.2, 0.3, 0.9])
    best = m.fit()
    assert m.iterators == 1
    assert m.order == [(w, k) for k in range(4) for w in ("train", "evaluate")]
    assert best is m.reports[1]
    assert m.logger.lines == ["metrics:".ljust(12) + "\t" + _Evaluator.metrics_str,
                              _line("epoch 0:", m.reports[0]), _line("epoch 1:", m.reports[1]),
                              _line("epoch 2:", m.reports[2]), _line("epoch 3:", m.reports[3]),
                              "early stop", _line("best:", m.reports[1])]
    assert m.logger.lines[2] == "epoch 1:    \t0.30000000  \t1.50000000  "         # the format itself


def test_fit_runs_every_epoch_without_a_stop(monkeypatch):
    m = _stub(monkeypatch, epochs=3, early_stop=0, ndcg=[0.3, 0.2, 0.1])          # patience <= 0: never
    best = m.fit()
    assert m.order == [(w, k) for k in range(3) for w in ("train", "evaluate")]
    assert best is m.reports[0]
    assert [l.split(":")[0] for l in m.logger.lines] == ["metrics", "epoch 0", "epoch 1", "epoch 2", "best"]
    assert m.logger.lines[-1] == _line("best:", m.reports[0])


def test_fit_without_epochs(monkeypatch):
    """the loop as it was before the models shared it: ``epochs=0`` makes the iterator, logs the header, trains and
    evaluates nothing and reports the ``best_result`` of a fresh ``EarlyStopping``: MetricReport(["None"], [0])"""
    m = _stub(monkeypatch, epochs=0, early_stop=2, ndcg=[])
    best = m.fit()
    assert m.iterators == 1 and m.order == []
    assert list(best.items()) == [("None", 0)]
    assert m.logger.lines == ["metrics:".ljust(12) + "\t" + _Evaluator.metrics_str, "best:".ljust(12) + "\t0.00000000  "]


def test_fit_logs_on_rank_0_only(monkeypatch):
    from skrec.parallel import DistContext
    m = _stub(monkeypatch, epochs=2, early_stop=0, ndcg=[0.1, 0.2])
    m.dist = DistContext(1, 2)
    assert m.fit() is m.reports[1] and m.logger.lines == []


# ---------------------------------------------------------------------------------------------------------------------
# 2. the order of the constructor's checks: limits and the one-GPU refusal come before the data set or the GPU is touched
#    (``run_config=None`` has no data set to read)
# ---------------------------------------------------------------------------------------------------------------------
# FPMC and TransRec have no limit that is checked before ``_build`` (the width of their rows is padded_width's there)
LIMITS = [("CDAE", dict(hidden_dim=128), NotImplementedError, "hidden_dim <= 64"),
          ("CDAE", dict(loss_func="square"), ValueError, "loss function 'square' is invalid"),
          ("MultVAE", dict(p_dims=[65]), NotImplementedError, "d <= 64"),
          ("MultVAE", dict(batch_size=2048), ValueError, "batch_size <= 1024"),
          ("HGN", dict(embed_size=65), NotImplementedError, "embed_size <= 64"),
          ("HGN", dict(seq_L=33), ValueError, "1 <= seq_L <= 32 and 1 <= seq_T <= 16"),
          ("HGN", dict(seq_T=17), ValueError, "1 <= seq_L <= 32 and 1 <= seq_T <= 16"),
          ("LightGCL", dict(d=128), NotImplementedError, "d <= 64"),
          ("DENS", dict(dim=128), NotImplementedError, "dim <= 64"),
          ("SelfCF", dict(embed_dim=128), NotImplementedError, "embed_dim <= 64"),
          ("BM3", dict(embed_dim=128), NotImplementedError, "embed_dim <= 64")]


@pytest.mark.parametrize("name,config,error,text", LIMITS, ids=[f"{c[0]}-{next(iter(c[1]))}" for c in LIMITS])
def test_limits_come_before_the_data_set(name, config, error, text):
    with pytest.raises(error, match=text):
        _cls(name)(None, config)


@pytest.mark.parametrize("name", ON_SCAFFOLD)
def test_one_gpu_refusal_comes_before_the_data_set(monkeypatch, name):
    import skrec.parallel as P
    monkeypatch.setattr(P, "init_from_env", lambda: P.DistContext(0, 2))         # no WORLD_SIZE: that would start a group
    with pytest.raises(NotImplementedError, match="runs on one GPU"):
        _cls(name)(None, {})


@pytest.mark.parametrize("name", ON_SCAFFOLD)
def test_detached_checks_the_limits_first(monkeypatch, name):
    """``detached`` refuses what the constructor refuses, before it asks for the GPU"""
    from skrec import _hip

    def no_gpu():
        raise AssertionError("the GPU is asked for before the limits are checked")
    monkeypatch.setattr(_hip, "require_gpu", no_gpu)
    for n, config, error, text in LIMITS:
        if n == name:
            with pytest.raises(error, match=text):
                _cls(name).detached(8, 8, config)


# ---------------------------------------------------------------------------------------------------------------------
# 3. one loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ON_SCAFFOLD + ("LightGCN", "LayerGCN"))
def test_no_model_has_a_loop_of_its_own(name):
    from skrec.recommender.base import DeviceRecommender
    assert _cls(name).fit is DeviceRecommender.fit
    assert "fit" not in vars(_cls(name))
