"""LDA-VB ``engine="native"`` on CPU tensors (``ops.lda_vb.estep_ref``, the CPU path of the
native engine): it computes what the torch engine computes at a fixed pass count, under both
strategies, and stops every document on its own when ``gamma_tol > 0``.

Tolerance 1e-9 relative: two torch summation orders of the same E-step differ by up to 8e-13
after 29 passes at these shapes, and 1e-9 is the bound of the existing cross-strategy test."""
import os

import pytest
import torch

from harp_amd.models import lda_vb as V
from harp_amd.ops import lda_vb as E
from harp_amd.parallel.comm import Communicator
from harp_amd.runtime.launcher import launch
from tests.test_lda_vb import _corpus
from tests.test_reference_datasets import golden

RTOL = 1e-9


def _close(a, b, what):
    err = ((a - b).abs() / b.abs().clamp_min(1e-300)).max() if a.numel() else 0.0
    assert float(err) <= RTOL, (what, float(err))


def _random_corpus(n_docs=40, vocab=300, seed=3):
    g = torch.Generator().manual_seed(seed)
    docs, words = [], []
    for d in range(n_docs):
        n = int(torch.randint(1, 60, (1,), generator=g))
        w = torch.randperm(vocab, generator=g)[:n].sort().values
        docs.append(torch.full((n,), d))
        words.append(w)
    doc, word = torch.cat(docs), torch.cat(words)
    return doc, word, torch.randint(1, 6, (doc.numel(),), generator=g).double()


def _cfg(K, engine, **kw):
    base = dict(num_topics=K, iterations=5, gamma_iters=29, gamma_tol=0.0, engine=engine, block=8)
    base.update(kw)
    return V.LDAVBConfig(**base)


def _compare_runs(a, b):
    _close(a["gamma"], b["gamma"], "gamma")
    _close(a["log_beta"], b["log_beta"], "log_beta")
    _close(a["alpha"], b["alpha"], "alpha")
    assert len(a["history"]) == len(b["history"])
    for ha, hb in zip(a["history"], b["history"]):
        assert abs(ha["elbo"] - hb["elbo"]) <= RTOL * abs(hb["elbo"]), (ha, hb)


@pytest.mark.parametrize("case", ["planted_k4", "random_k65"])
def test_fixed_passes_native_equals_torch(case):
    if case == "planted_k4":
        (d, w, c), nd, vocab, K = _corpus(), 60, 40, 4
    else:
        (d, w, c), nd, vocab, K = _random_corpus(), 40, 300, 65
    nat = V.train_lda_vb(Communicator(), d, w, c, nd, vocab, _cfg(K, "native"))
    ref = V.train_lda_vb(Communicator(), d, w, c, nd, vocab, _cfg(K, "torch"))
    _compare_runs(nat, ref)
    assert nat["log_beta"].shape == (K, vocab) and nat["gamma"].shape == (nd, K)
    assert all(h["passes_max"] == 29 for h in nat["history"])
    assert all("passes_max" not in h for h in ref["history"])


def _job(comm, d, w, c, strategy):
    P, r = comm.world_size, comm.rank
    m = (d % P) == r
    out = V.train_lda_vb(comm, d[m] // P, w[m], c[m], int((d[m] // P).max() + 1), 40, _cfg(4, "native", strategy=strategy))
    return out["gamma"], [h["elbo"] for h in out["history"]], out["log_beta"]


def test_native_strategies_agree_with_single_worker():
    d, w, c = _corpus()
    single = V.train_lda_vb(Communicator(), d, w, c, 60, 40, _cfg(4, "native"))
    for strategy in ("allreduce", "push_pull"):
        res = launch(_job, 2, args=(d, w, c, strategy), timeout=300)
        for r, (gamma, elbo, log_beta) in enumerate(res):
            _close(gamma, single["gamma"][r::2], strategy + " gamma")
            if strategy == "allreduce":  # push_pull leaves word blocks a worker never reads at zero
                _close(log_beta, single["log_beta"], strategy + " log_beta")
            for e, h in zip(elbo, single["history"]):
                assert abs(e - h["elbo"]) <= RTOL * abs(h["elbo"])


def _stopping_inputs():
    d, w, c = _corpus()
    keep = d != 7  # document 7 has no terms
    d, w, c = d[keep], w[keep], c[keep]
    g = torch.Generator().manual_seed(5)
    beta = torch.rand((4, 40), generator=g, dtype=torch.float64) + 0.05
    for t in range(4):  # every planted topic has a beta row to lock on to: 8 to 10 passes per document
        beta[t, t * 10:(t + 1) * 10] += 1.0
    return d, w, c, (beta / beta.sum(1, keepdim=True)).log(), torch.full((4,), 0.1, dtype=torch.float64)


def test_per_document_stopping():
    d, w, c, log_beta, alpha = _stopping_inputs()
    plan = E.DocPlan.build(d, w, 60)
    gamma, passes, doc_ll, S_t = E.estep(plan, c, log_beta.t().contiguous(), alpha, 200, 1e-6)
    assert passes.dtype == torch.int32 and passes.shape == (60,)
    assert int(passes.min()) >= 1 and int(passes.max()) < 200
    assert passes.unique().numel() > 1, "every document stopped after the same pass"
    assert int(passes[7]) == 1 and torch.equal(gamma[7], alpha) and float(doc_ll[7]) == 0.0
    # the torch engine runs all documents until the slowest one has met the tolerance
    n_torch = 0
    cfg = V.LDAVBConfig(num_topics=4, gamma_iters=200, gamma_tol=1e-6)
    orig = torch.softmax

    def counting(*a, **k):
        nonlocal n_torch
        n_torch += 1
        return orig(*a, **k)

    torch.softmax = counting
    try:
        g_t, _, _ = V._estep(d, w, c, 60, log_beta, alpha, cfg)
    finally:
        torch.softmax = orig
    assert 1 <= n_torch < 200
    assert int(passes.max()) <= n_torch
    # both stopped within tol of the same fixed point
    assert float((gamma - g_t).abs().max()) < 1e-3
    assert abs(float(S_t.sum()) - float(c.sum())) <= 1e-10 * float(c.sum())


def test_unsorted_input_equals_sorted():
    d, w, c = _corpus()
    p = torch.randperm(d.numel(), generator=torch.Generator().manual_seed(1))
    a = V.train_lda_vb(Communicator(), d, w, c, 60, 40, _cfg(4, "native", iterations=3))
    b = V.train_lda_vb(Communicator(), d[p], w[p], c[p], 60, 40, _cfg(4, "native", iterations=3))
    plan = E.DocPlan.build(d[p], w[p], 60)
    assert plan.perm is not None and E.DocPlan.build(d, w, 60).perm is None
    assert bool((plan.doc[1:] >= plan.doc[:-1]).all())
    _compare_runs(b, a)


def test_plan_schedule_is_longest_first():
    lengths = [0, 3, E.LONG_DOC_TERMS + 1, 1, E.LONG_DOC_TERMS, 2 * E.LONG_DOC_TERMS]
    d = torch.cat([torch.full((n,), i) for i, n in enumerate(lengths)])
    plan = E.DocPlan.build(d, torch.zeros_like(d), len(lengths))
    assert plan.sched.tolist() == [5, 2, 4, 1, 3, 0]
    assert plan.n_long == 2 and plan.long_docs.tolist() == [5, 2]
    assert plan.rowptr.tolist()[-1] == sum(lengths) and plan.word.dtype == torch.int32
    assert [E.group_width(k) for k in (1, 2, 3, 8, 9, 32, 33, 1024)] == [2, 2, 4, 8, 16, 32, 64, 64]


def test_bad_engine_and_too_many_topics_raise():
    d, w, c = _corpus()
    with pytest.raises(ValueError, match="engine"):
        V.train_lda_vb(Communicator(), d, w, c, 60, 40, _cfg(4, "bogus"))
    with pytest.raises(ValueError, match=str(E.MAX_TOPICS)):
        V.train_lda_vb(Communicator(), d, w, c, 60, 40, _cfg(E.MAX_TOPICS + 1, "native", iterations=1))


def test_cli_engines_write_the_same_likelihood(tmp_path):
    from harp_amd import cli

    d = golden("tutorial", "lda-cvb", "sample-sparse-data")
    ll = {}
    for engine in ("native", "torch"):
        out = tmp_path / engine
        assert cli.main(["ldacvb", d, os.path.join(d, "sample-sparse-metadata"), str(out), "11", "2", "12", "1", "5",
                         "1", "1", "--backend", "gloo", "--engine", engine]) == 0
        ll[engine] = [float(ln.split()[1]) for ln in (out / "likelihood").read_text().splitlines()]
    assert len(ll["native"]) == 5
    for a, b in zip(ll["native"], ll["torch"]):
        assert abs(a - b) <= RTOL * abs(b), (a, b)
