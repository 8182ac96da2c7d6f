"""Fused MLP epilogues (csrc/nn.hip) vs the fp64 torch formulation of the same gradient."""
import pytest
import torch

from harp_amd.models.nn import MLP
from harp_amd.ops import nn as NO

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("act", ["sigmoid", "tanh", "relu"])
@pytest.mark.parametrize("sizes,b", [([20, 32, 10], 64), ([784, 300, 100, 10], 257), ([5, 7, 3000], 33)])
def test_native_gradient_matches_fp64(cuda, act, sizes, b):
    net = MLP(sizes, activation=act, device=cuda, seed=4)
    ref = MLP(sizes, activation=act, device="cpu", dtype=torch.float64, seed=4)
    ref.flat.copy_(net.flat.double().cpu())
    g = torch.Generator().manual_seed(1)
    X = torch.randn(b, sizes[0], generator=g)
    y = torch.randint(0, sizes[-1], (b,), generator=g)
    Y = torch.nn.functional.one_hot(y, sizes[-1])
    assert net._native(X.to(cuda))
    got = net.gradient(X.to(cuda), Y.to(cuda)).double().cpu()
    want = ref.gradient(X.double(), Y)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-6), (got - want).abs().max()
    loss_ref = float(-(torch.log_softmax(ref.forward(X.double())[-2] @ ref.params[-2].t() + ref.params[-1], 1)
                       .gather(1, y[:, None])).sum())
    assert float(net.last_loss) == pytest.approx(loss_ref, rel=1e-4)


def test_softmax_xent_kernel(cuda):
    z = torch.randn(100, 37, device=cuda)
    lab = torch.randint(0, 37, (100,), device=cuda, dtype=torch.int32)
    delta = torch.empty_like(z)
    db = torch.zeros(37, device=cuda)
    loss = NO.softmax_xent(z, lab, 0.5, delta, db)
    p = torch.softmax(z.double(), 1)
    want = (p - torch.nn.functional.one_hot(lab.long(), 37)) * 0.5
    assert torch.allclose(delta.double(), want, atol=1e-6)
    assert torch.allclose(db.double(), want.sum(0), atol=1e-5)
    assert float(loss) == pytest.approx(float(-torch.log(p.gather(1, lab.long()[:, None])).sum()), rel=1e-5)


# ---------------------------------------------------------------------------------------
# The three epilogue kernels called directly at their tile edges. All data comes from local
# generators; the references are fp64 torch on the same fp32 inputs.
def _xent_ref(z, lab, scale):
    """(delta, column sums, summed loss) in fp64; a label outside [0, C) has no target and
    no loss. The loss goes through log_softmax: -log(softmax) is inf where p underflows."""
    C = z.shape[1]
    zd, lab = z.double().cpu(), lab.long().cpu()
    ok = (lab >= 0) & (lab < C)
    onehot = torch.zeros_like(zd)
    onehot[ok, lab[ok]] = 1.0
    delta = (torch.softmax(zd, 1) - onehot) * scale
    loss = -torch.log_softmax(zd, 1)[ok, lab[ok]].sum()
    return delta, delta.sum(0), float(loss)


def _xent_check(cuda, z, lab, scale, g, delta_atol=1e-6, dbias_atol=1e-5, loss_rel=1e-5):
    B, C = z.shape
    want, wsum, wloss = _xent_ref(z, lab, scale)
    zg, lg = z.to(cuda), lab.to(cuda)
    d0 = torch.full_like(zg, float("nan"))
    loss0 = NO.softmax_xent(zg, lg, scale, d0, None)  # no bias gradient: delta and loss still right
    old = torch.randn(C, generator=g)
    d1, db = torch.full_like(zg, float("nan")), old.to(cuda)
    loss1 = NO.softmax_xent(zg, lg, scale, d1, db)  # accumulates into a pre-filled dbias
    for delta, loss in ((d0, loss0), (d1, loss1)):
        assert torch.isfinite(delta).all() and torch.isfinite(loss)
        assert torch.allclose(delta.double().cpu(), want, rtol=0, atol=delta_atol), (delta.double().cpu() - want).abs().max()
        assert abs(float(loss) - wloss) <= loss_rel * abs(wloss), (float(loss), wloss)
    assert torch.allclose(db.double().cpu(), old.double() + wsum, rtol=0, atol=dbias_atol)
    return d1


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 257])
def test_softmax_xent_shapes(cuda, C, B):
    """C below, at and above one wave and C = 1; B = 1, 3 and 5 leave rows past B in the last
    4-row workgroup."""
    g = torch.Generator().manual_seed(100 * C + B)
    z = torch.randn(B, C, generator=g)
    lab = torch.randint(0, C, (B,), generator=g, dtype=torch.int32)
    _xent_check(cuda, z, lab, 0.5, g)


def _hard_logits():
    g = torch.Generator().manual_seed(11)
    C = 70
    z = torch.randn(9, C, generator=g)
    z[:4] *= 80.0          # needs the max subtraction: exp(z) overflows fp32 beyond 88
    z[4] = 3.25            # all equal
    z[5] = z[6]
    z[5, 17] += 1e4        # one logit far above the rest, with the right and a wrong label
    z[6, 17] += 1e4
    lab = torch.randint(0, C, (9,), generator=g, dtype=torch.int32)
    lab[5], lab[6] = 17, 3
    lab[7], lab[8] = -1, C  # out of range: no target, no loss
    return z, lab, g


def test_softmax_xent_large_logits_and_bad_labels(cuda):
    """Measured on the CPU for this batch, torch's own fp32 softmax / log_softmax against fp64:
    softmax 5.59e-08 absolute, summed loss (10825.36) 3.24e-08 relative. Four times either is
    below the standing tolerances (delta 1e-6, loss 1e-5 relative), so those stay."""
    z, lab, g = _hard_logits()
    scale = 0.25
    delta = _xent_check(cuda, z, lab, scale, g).double().cpu()
    rows = delta.sum(1)
    assert rows[:7].abs().max().item() <= 1e-5 * scale      # a target: the row sums to 0
    assert (rows[7:] - scale).abs().max().item() <= 1e-5 * scale  # none: softmax * scale
    assert torch.allclose(delta[7:], torch.softmax(z[7:].double(), 1) * scale, rtol=0, atol=1e-6)


def test_softmax_xent_class_cap(cuda):
    """The launcher takes C <= 16384 and asks for 4 C bytes of dynamic LDS beside the
    kernel's 16 static bytes. Where that fits the device's workgroup limit the cap must
    work; where it does not, the launcher must refuse it (bad argument) and never fail a
    launch."""
    C, B, static_lds = 16384, 5, 16
    limit = torch.cuda.get_device_properties(cuda).shared_memory_per_block
    fits = 4 * C + static_lds <= limit
    print(f"shared memory per workgroup {limit} B, softmax_xent at C = {C} needs {4 * C + static_lds} B")
    g = torch.Generator().manual_seed(5)
    z = torch.randn(B, C, generator=g)
    lab = torch.randint(0, C, (B,), generator=g, dtype=torch.int32)
    if fits:
        _xent_check(cuda, z, lab, 0.5, g)
    else:
        with pytest.raises(RuntimeError, match="bad argument"):
            NO.softmax_xent(z.to(cuda), lab.to(cuda), 0.5, torch.empty(B, C, device=cuda), None)
        top = (limit - static_lds) // 4  # the widest row that fits must still work
        _xent_check(cuda, z[:, :top].contiguous(), lab % top, 0.5, g)


_ACT64 = {"sigmoid": torch.sigmoid, "tanh": torch.tanh, "relu": torch.relu, "none": lambda t: t}
# one fp32 rounding of z + b (2^-24 relative, |z + b| < 8 here) and a few ulp of an output of
# magnitude <= 1 for sigmoid / tanh; relu and "none" return the rounded sum itself
_ACT_RTOL, _ACT_ATOL = 2.0 ** -23, 1e-6


@pytest.mark.parametrize("rows", [1, 33])
@pytest.mark.parametrize("N", [1, 255, 257])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("act", ["sigmoid", "tanh", "relu", "none"])
def test_bias_act_direct(cuda, act, with_bias, N, rows):
    g = torch.Generator().manual_seed(rows * 1000 + N)
    z = torch.randn(rows, N, generator=g)
    b = torch.randn(N, generator=g) if with_bias else None
    want = _ACT64[act](z.double() + (b.double() if with_bias else 0.0))
    out = NO.bias_act_(z.to(cuda), b.to(cuda) if with_bias else None, act)
    assert torch.allclose(out.double().cpu(), want, rtol=_ACT_RTOL, atol=_ACT_ATOL)


def test_bias_act_saturates_exactly(cuda):
    z = torch.tensor([[100.0, -100.0, 50.0, -50.0]])
    s = NO.bias_act_(z.to(cuda), None, "sigmoid").cpu()
    assert s[0, :2].tolist() == [1.0, 0.0] and not torch.isnan(s).any()
    t = NO.bias_act_(z.to(cuda), None, "tanh").cpu()
    assert t[0, 2:].tolist() == [1.0, -1.0] and t[0, :2].tolist() == [1.0, -1.0]
    b = torch.tensor([60.0, -60.0, 0.0, 0.0])  # saturated by the bias
    s = NO.bias_act_(torch.full((1, 4), 40.0).to(cuda) * torch.tensor([1.0, -1.0, 1.0, -1.0], device=cuda),
                     b.to(cuda), "sigmoid").cpu()
    assert s[0, :2].tolist() == [1.0, 0.0] and not torch.isnan(s).any()


def test_bias_act_grid_stride(cuda):
    """65537 x 257 elements are more than 65536 blocks of 256: the grid-stride loop runs."""
    rows, N = 65537, 257
    assert (rows * N + 255) // 256 > 65536
    g = torch.Generator().manual_seed(9)
    z = torch.randn(rows, N, generator=g).to(cuda)
    b = torch.randn(N, generator=g).to(cuda)
    want = torch.tanh(z.double() + b.double())
    out = NO.bias_act_(z, b, "tanh")
    assert torch.allclose(out.double(), want, rtol=_ACT_RTOL, atol=_ACT_ATOL)


_DACT64 = {"sigmoid": lambda a: a * (1 - a), "tanh": lambda a: 1 - a * a, "relu": lambda a: (a > 0).double()}


@pytest.mark.parametrize("N", [1, 255, 256, 257])
@pytest.mark.parametrize("B", [1, 31, 32, 33])
@pytest.mark.parametrize("act", ["sigmoid", "tanh", "relu"])
def test_dact_bgrad_direct(cuda, act, B, N):
    """The 32-row and 256-column tile edges, without a bias gradient and with a pre-filled one."""
    g = torch.Generator().manual_seed(B * 1000 + N)
    a = _ACT64[act](torch.randn(B, N, generator=g))  # activation values, zeros included for relu
    delta = torch.randn(B, N, generator=g)
    want = delta.double() * _DACT64[act](a.double())
    d0 = NO.dact_bgrad_(delta.to(cuda), a.to(cuda), act, None)
    assert torch.allclose(d0.double().cpu(), want, rtol=0, atol=1e-6)
    old = torch.randn(N, generator=g)
    db = old.to(cuda)
    d1 = NO.dact_bgrad_(delta.to(cuda), a.to(cuda), act, db)
    assert torch.equal(d1, d0)
    assert torch.allclose(db.double().cpu(), old.double() + want.sum(0), rtol=0, atol=1e-5)
