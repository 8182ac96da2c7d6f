"""Native fp64 EM-GMM (csrc/gmm_f64.hip) against plain fp64 torch on the CPU."""
import math

import pytest
import torch

from harp_amd.models import kernels as KM
from harp_amd.ops import gmm_f64 as GF

pytestmark = pytest.mark.gpu
CH = GF.CHUNK


def _planted(n, d, K, dtype, seed):
    """Cluster k sits at 64 k e_0 with integer offsets in [-2, 2]: every competing log p is at
    least 1800 below the winner's, so every r is exactly 0 or 1 and all statistics are sums of
    small integers. The reference takes the rows as the dtype holds them (still integers)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.arange(n) % K
    mu = torch.zeros(K, d, dtype=torch.float64)
    mu[:, 0] = 64.0 * torch.arange(K)
    X = (mu[z] + torch.randint(-2, 3, (n, d), generator=g).double()).to(dtype)
    return X, z, mu


# n, d, K, splits, dtype, extra row stride
EXACT = [(1, 1, 1, 1, torch.float64, 0), (15, 3, 7, 1, torch.float32, 0), (17, 16, 8, 3, torch.bfloat16, 0),
         (CH - 1, 17, 9, 1, torch.float64, 0), (CH + 1, 32, 17, 3, torch.float32, 0),
         (2 * CH + 1, 33, 8, 3, torch.float64, 0), (2 * CH + 1, 48, 9, 1, torch.bfloat16, 0),
         (2 * CH + 1, 64, 17, 3, torch.float64, 0), (CH + 1, 64, 7, 1, torch.float32, 5),
         (2 * CH + 1, 16, 17, 1, torch.float64, 3)]


@pytest.mark.parametrize("n,d,K,splits,dtype,pad", EXACT)
def test_exact_on_separated_integer_clusters(cuda, n, d, K, splits, dtype, pad):
    X, z, mu = _planted(n, d, K, dtype, n + 100 * d + K)
    Xd = X.double()
    Xg = torch.zeros((n, d + pad), dtype=dtype).to(cuda)[:, :d]
    Xg.copy_(X)
    w = torch.full((K,), 1.0 / K, dtype=torch.float64)
    cov = torch.eye(d, dtype=torch.float64).expand(K, d, d).contiguous()
    N, S1, S2, ll = GF.estep_stats(Xg, w.to(cuda), mu.to(cuda), cov.to(cuda), "full", splits=splits)
    assert torch.equal(N.cpu(), torch.bincount(z, minlength=K).double())
    assert torch.equal(S1.cpu(), torch.zeros(K, d, dtype=torch.float64).index_add_(0, z, Xd))
    ref2 = torch.stack([Xd[z == k].t() @ Xd[z == k] for k in range(K)])
    assert torch.equal(S2.cpu(), ref2)
    lse = math.log(1.0 / K) - 0.5 * d * math.log(2 * math.pi) - 0.5 * ((Xd - mu[z]) ** 2).sum(1)
    assert abs(ll.item() - lse.sum().item()) <= n * 2.0 ** -52 * lse.abs().sum().item()
    assert torch.equal(GF.predict(Xg, w.to(cuda), mu.to(cuda), cov.to(cuda), "full").cpu(), z)


def _mixture(n, d, K, seed):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(K, d, generator=g, dtype=torch.float64) * 3
    A = torch.randn(K, d, d, generator=g, dtype=torch.float64) * 0.3
    cov = A @ A.transpose(1, 2) + torch.eye(d, dtype=torch.float64)
    w = torch.rand(K, generator=g, dtype=torch.float64) + 0.5
    w = w / w.sum()
    z = torch.randint(0, K, (n,), generator=g)
    L = torch.linalg.cholesky(cov)
    X = mu[z] + (L[z] @ torch.randn(n, d, 1, generator=g, dtype=torch.float64)).squeeze(-1)
    return X, w, mu, cov


def _reference(X, w, mu, cov, kind):
    logp = KM._log_gauss(X, mu, cov, kind) + torch.log(w)[None, :]
    lse = torch.logsumexp(logp, 1)
    R = torch.exp(logp - lse[:, None])
    S2 = torch.einsum("nk,ni,nj->kij", R, X, X) if kind == "full" else R.t() @ (X * X)
    return R.sum(0), R.t() @ X, S2, lse.sum()


def _close(got, ref):
    N, S1, S2, ll = (t.cpu() for t in got)
    return (torch.allclose(N, ref[0], rtol=1e-9, atol=1e-6) and torch.allclose(S1, ref[1], rtol=1e-9, atol=1e-6)
            and torch.allclose(S2, ref[2], rtol=1e-9, atol=1e-5) and abs(ll.item() - ref[3].item()) <= 1e-9 * abs(ref[3].item()))


@pytest.mark.parametrize("d,K,kind", [(5, 3, "full"), (17, 9, "full"), (64, 5, "full"), (12, 9, "diag")])
def test_one_step_matches_fp64_torch_and_repeats(cuda, d, K, kind):
    X, w, mu, cov = _mixture(2000, d, K, d * 100 + K)
    if kind == "diag":
        cov = torch.diagonal(cov, dim1=1, dim2=2).contiguous()
    ref = _reference(X, w, mu, cov, kind)
    args = [t.to(cuda) for t in (X, w, mu, cov)]
    one, again, three = GF.estep_stats(*args, kind, splits=1), GF.estep_stats(*args, kind, splits=1), \
        GF.estep_stats(*args, kind, splits=3)
    assert _close(one, ref) and _close(three, ref) and _close(GF.estep_stats(*args, kind), ref)
    assert all(torch.equal(a, b) for a, b in zip(one, again))
    assert kind == "diag" or torch.equal(one[2], one[2].transpose(1, 2))  # mirrored, not recomputed


def test_no_buffer_of_n_times_k(cuda):
    n, d, K = 262144, 8, 64
    X, w, mu, cov = _mixture(n, d, K, 11)
    args = [t.to(cuda) for t in (X, w, mu, cov)]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = GF.estep_stats(*args, "full")
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < n * K * 8 // 4
    assert abs(out[0].sum().item() - n) < 1e-6 * n


def test_em_and_predict_end_to_end(cuda):
    X, w, mu, cov = _mixture(30000, 6, 4, 1)
    init = {"weights": w, "means": mu + 0.5, "covariances": cov}
    kw = dict(n_iterations=25, accuracy_threshold=0, init=init)
    a = KM.em_gmm(X.to(cuda), 4, engine="native", **kw)
    b = KM.em_gmm(X.to(cuda), 4, engine="torch", **kw)
    assert torch.allclose(a["means"], b["means"], rtol=1e-8, atol=1e-8)
    assert torch.allclose(a["covariances"], b["covariances"], rtol=1e-8, atol=1e-8)
    assert abs(float(a["loglik"]) - float(b["loglik"])) < 1e-9 * abs(float(b["loglik"]))
    # fp32 rows are widened in registers: the same bits as the rows widened beforehand
    X32 = X.float().to(cuda)
    c, e = KM.em_gmm(X32, 4, engine="native", **kw), KM.em_gmm(X32.double(), 4, engine="native", **kw)
    assert all(torch.equal(c[k], e[k]) for k in ("weights", "means", "covariances", "loglik"))
    # labels, wherever the two best log-densities are further apart than rounding
    model = {k: v.cpu() for k, v in a.items() if isinstance(v, torch.Tensor)}
    top = (KM._log_gauss(X, model["means"], model["covariances"], "full") + torch.log(model["weights"])[None]).topk(2, 1)
    clear = (top.values[:, 0] - top.values[:, 1]) > 1e-9
    assert clear.double().mean().item() >= 0.99
    got = KM.gmm_predict(X.to(cuda), a, engine="native").cpu()
    assert got.dtype == torch.int64 and torch.equal(got[clear], top.indices[clear, 0])
    assert torch.equal(got[clear], KM.gmm_predict(X.to(cuda), a, engine="torch").cpu()[clear])
