"""GPU WDA-MDS row kernels (csrc/mds.hip) vs the fp64 torch formulas on the CPU."""
import math

import pytest
import torch

from harp_amd.models import mds as MD
from harp_amd.parallel.comm import Communicator

pytestmark = pytest.mark.gpu


def _direct_rows(D, W, row0, X, diff):
    """B(Z) X and the stress of the rows with distances from coordinate differences, as the
    kernel forms them. The model's CPU path takes them from the Gram matrix, which loses
    |x|^2 * 2^-52 / d_ij^2: nothing at dim >= 2 here (closest pair 1e-3), but 1e-6 of a
    B(Z) X entry at dim = 1, where 700 points on a line have pairs 2e-6 apart."""
    n_r = D.shape[0]
    Xr = X[row0:row0 + n_r]
    Dz = (Xr[:, None, :] - X[None, :, :]).pow(2).sum(-1).sqrt()
    off = torch.ones_like(Dz, dtype=torch.bool)
    off[torch.arange(n_r), torch.arange(n_r) + row0] = False
    ok = off & (W != 0) & (Dz >= 1e-10) & (D > diff)
    B = torch.where(ok, -W * (D - diff) / Dz.clamp_min(1e-10), torch.zeros_like(Dz))
    bc = B @ X - B.sum(1, keepdim=True) * Xr
    dd = D - diff - Dz
    return bc, (W * dd * dd * ((W != 0) & (D >= diff))).sum()


@pytest.mark.parametrize("dim", [1, 2, 3, 4])
@pytest.mark.parametrize("T", [0.0, 0.05])
def test_bc_and_stress_match_torch(cuda, dim, T):
    g = torch.Generator().manual_seed(dim)
    n, row0, n_r = 700, 200, 300
    Y = torch.rand(n, dim, generator=g, dtype=torch.float64)
    D = MD.quantize_distances(torch.cdist(Y, Y))[row0:row0 + n_r].contiguous()
    W = (torch.rand(n_r, n, generator=g, dtype=torch.float64) < 0.9).double()
    X = torch.rand(n, dim, generator=g, dtype=torch.float64)
    X[5] = X[row0 + 3]  # a coincident pair (d_ij < 1e-10 branch)
    comm = Communicator()
    cpu = MD._Rows(comm, D, W, row0)
    gpu = MD._Rows(Communicator(None, cuda), D.to(cuda), W.to(cuda), row0)
    assert gpu._native(X.to(cuda))
    bc, s = gpu.bc(X.to(cuda), T, dim).cpu(), gpu.stress(X.to(cuda), T, dim).cpu()
    bc_dir, s_dir = _direct_rows(D, W, row0, X, math.sqrt(2.0 * dim) * T if T > 1e-9 else 0.0)
    assert torch.allclose(bc, bc_dir, rtol=1e-9, atol=1e-9 * bc_dir.abs().max().item())
    assert math.isclose(float(s), float(s_dir), rel_tol=1e-9)
    s_ref = cpu.stress(X, T, dim)
    assert math.isclose(float(s), float(s_ref), rel_tol=1e-9)
    if dim >= 2:  # see _direct_rows: at dim = 1 the CPU path itself is 1e-6 off
        bc_ref = cpu.bc(X, T, dim)
        assert torch.allclose(bc, bc_ref, rtol=1e-9, atol=1e-9 * bc_ref.abs().max().item())


def test_wdamds_gpu_equals_cpu(cuda):
    g = torch.Generator().manual_seed(0)
    Y = torch.rand(60, 3, generator=g, dtype=torch.float64)
    D = MD.quantize_distances(torch.cdist(Y, Y))
    W = torch.ones(60, 60, dtype=torch.float64)
    cfg = MD.MDSConfig(d=3, alpha=0.9, threshold=1e-7)
    ref = MD.wda_mds(Communicator(), D, W, 0, 60, cfg)
    out = MD.wda_mds(Communicator(None, cuda), D, W, 0, 60, cfg)
    assert out["stress"] < 1e-3
    assert abs(out["stress"] - ref["stress"]) < 1e-6
    assert torch.allclose(torch.cdist(out["X"].cpu(), out["X"].cpu()), D, atol=0.05)
