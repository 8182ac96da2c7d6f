"""The native LDA-VB E-step (``csrc/lda_vb.hip``) on the device against its torch reference
``ops.lda_vb.estep_ref`` on the CPU: the device digamma, every lane mapping (sub-wave groups of
2..32 lanes, one wave with 1..16 values per lane) across short, long and empty documents,
per-document stopping, the memory model and a training run end to end."""
import pytest
import torch

from harp_amd.models import lda_vb as V
from harp_amd.ops import lda_vb as E
from harp_amd.parallel.comm import Communicator
from tests.test_lda_vb import _corpus

pytestmark = pytest.mark.gpu

KS = [1, 2, 8, 9, 16, 17, 32, 33, 63, 64, 65, 130, 1024]
VOCAB = 2000
L = E.LONG_DOC_TERMS


def test_digamma_against_torch(cuda):
    x = torch.cat([torch.logspace(-6, 6, 200000, dtype=torch.float64),
                   torch.linspace(1.3, 1.6, 20000, dtype=torch.float64)])
    ref = torch.digamma(x)
    got = E.digamma(x.to(cuda)).cpu()
    err = (got - ref).abs() / ref.abs().clamp_min(1.0)
    i = int(err.argmax())
    print(f"digamma: max error {float(err[i]):.3e} x max(1, |psi|) at x = {float(x[i]):.6g}")
    assert bool(torch.isfinite(got).all())
    assert float(err[i]) <= 4e-15


@pytest.fixture(scope="module")
def corpus():
    """One corpus for every K: the lengths straddle the wave width and LONG_DOC_TERMS, word 0
    is in every second document (a hot row for the atomics), counts are in 1..5."""
    g = torch.Generator().manual_seed(11)
    lengths = [0, 1, 2, 63, 64, 65, L - 1, L, L + 1, 4 * L] + torch.randint(1, 120, (40,), generator=g).tolist()
    lengths = [lengths[i] for i in torch.randperm(len(lengths), generator=g).tolist()]
    docs, words = [], []
    for d, n in enumerate(lengths):
        w = torch.randperm(VOCAB - 1, generator=g)[:n] + 1
        if d % 2 == 0 and n:
            w[0] = 0
        docs.append(torch.full((n,), d))
        words.append(w.sort().values)
    doc, word = torch.cat(docs), torch.cat(words)
    cnt = torch.randint(1, 6, (doc.numel(),), generator=g).double()
    return E.DocPlan.build(doc, word, len(lengths)), cnt, lengths


def _model(K):
    """log_beta_t [V, K] with 20 % of the entries -inf, but never a whole word."""
    g = torch.Generator().manual_seed(100 + K)
    beta = torch.rand((K, VOCAB), generator=g, dtype=torch.float64) + 0.05
    lbt = (beta / beta.sum(1, keepdim=True)).log().t().contiguous()
    dead = torch.rand((VOCAB, K), generator=g) < 0.2
    dead[torch.arange(VOCAB), torch.randint(0, K, (VOCAB,), generator=g)] = False
    lbt[dead] = -float("inf")
    return lbt, torch.full((K,), 0.1, dtype=torch.float64)


def _on(plan, dev):
    return E.DocPlan(plan.rowptr.to(dev), plan.word.to(dev), plan.doc.to(dev), plan.sched.to(dev), plan.n_docs,
                     plan.n_long, plan.max_word, None if plan.perm is None else plan.perm.to(dev))


def _rel(a, b, atol=0.0):
    return float(((a - b).abs() - atol).clamp_min(0.0).div(b.abs().clamp_min(1e-300)).max())


@pytest.mark.parametrize("K", KS)
def test_estep_fixed_passes(cuda, corpus, K):
    plan, cnt, lengths = corpus
    assert plan.n_long == 2 and plan.sched[0] == lengths.index(4 * L)
    lbt, alpha = _model(K)
    g_r, p_r, ll_r, S_r = E.estep_ref(plan, cnt, lbt, alpha, 29, 0.0)
    g, p, ll, S = (t.cpu() for t in E.estep(_on(plan, cuda), cnt.to(cuda), lbt.to(cuda), alpha.to(cuda), 29, 0.0))
    for t in (g_r, ll_r, S_r, g, ll, S):
        assert bool(torch.isfinite(t).all())
    errs = (_rel(g, g_r), _rel(ll, ll_r), _rel(S, S_r, 1e-12), abs(float(S.sum()) - float(cnt.sum())) / float(cnt.sum()))
    print(f"K={K}: gamma {errs[0]:.2e} doc_ll {errs[1]:.2e} S_t {errs[2]:.2e} mass {errs[3]:.2e}")
    assert torch.equal(p, p_r)
    empty = lengths.index(0)
    assert int(p[empty]) == 1 and torch.equal(g[empty], alpha) and float(ll[empty]) == 0.0
    assert all(int(p[d]) == 29 for d in range(len(lengths)) if d != empty)
    assert errs[0] <= 1e-9 and errs[1] <= 1e-9 and errs[2] <= 1e-9
    assert errs[3] <= 1e-10
    assert bool((S[lbt == -float("inf")] == 0).all()), "a -inf entry must give phi == 0 exactly"


@pytest.mark.parametrize("K", KS)
def test_estep_per_document_stopping(cuda, corpus, K):
    plan, cnt, lengths = corpus
    lbt, alpha = _model(K)
    tol = 1e-6
    trace = []
    g_r, p_r, _, _ = E.estep_ref(plan, cnt, lbt, alpha, 200, tol, trace=trace)
    margin = float(((torch.cat(trace) - tol).abs() / tol).min())
    print(f"K={K}: closest pass delta to tol {margin:.2e} relative, passes {int(p_r.min())}..{int(p_r.max())}")
    assert margin > 1e-6, "a reference pass delta sits on the stopping threshold: passes could differ by rounding"
    g, p, _, _ = (t.cpu() for t in E.estep(_on(plan, cuda), cnt.to(cuda), lbt.to(cuda), alpha.to(cuda), 200, tol))
    assert torch.equal(p, p_r)
    assert _rel(g, g_r) <= 1e-9


def test_memory_stays_at_the_outputs(cuda):
    """D = 2000, V = 5000, K = 256, about 2e5 pairs: one [nnz, K] fp64 matrix would be 410 MB, the
    engine's outputs (gamma, S_t, passes, doc_ll) are about 15 MB."""
    g = torch.Generator().manual_seed(2)
    D, Vc, K = 2000, 5000, 256
    doc = torch.arange(D).repeat_interleave(100)
    word = torch.randint(0, Vc, (doc.numel(),), generator=g)
    cnt = torch.randint(1, 6, (doc.numel(),), generator=g).double().to(cuda)
    plan = _on(E.DocPlan.build(doc, word, D), cuda)
    beta = torch.rand((Vc, K), generator=g, dtype=torch.float64) + 0.05
    lbt = (beta / beta.sum(0, keepdim=True)).log().to(cuda)
    alpha = torch.full((K,), 0.1, dtype=torch.float64, device=cuda)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(cuda)
    base = torch.cuda.memory_allocated(cuda)
    out = E.estep(plan, cnt, lbt, alpha, 5, 0.0)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(cuda) - base
    print(f"estep peak above the inputs: {extra / 1e6:.1f} MB")
    assert extra < 100e6
    assert abs(float(out[3].sum()) - float(cnt.sum())) <= 1e-10 * float(cnt.sum())


def test_train_native_on_device_equals_torch_on_cpu(cuda):
    d, w, c = _corpus()
    kw = dict(num_topics=4, iterations=5, gamma_iters=29, gamma_tol=0.0)
    ref = V.train_lda_vb(Communicator(device="cpu"), d, w, c, 60, 40, V.LDAVBConfig(engine="torch", **kw))
    nat = V.train_lda_vb(Communicator(device=cuda), d, w, c, 60, 40, V.LDAVBConfig(engine="native", **kw))
    assert nat["gamma"].device.type == "cuda" and nat["log_beta"].shape == (4, 40)
    for a, b in zip(nat["history"], ref["history"]):
        assert abs(a["elbo"] - b["elbo"]) <= 1e-9 * abs(b["elbo"]), (a, b)
        assert a["passes_max"] == 29
    B = nat["log_beta"].exp().cpu()
    for t in range(4):
        assert B[:, t * 10:(t + 1) * 10].sum(1).max() > 0.9
