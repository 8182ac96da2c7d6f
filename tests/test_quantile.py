"""Exact quantiles by radix select on the CPU (the torch mirror of csrc/quantile.hip in
ops/quantile.py; the kernels are checked against it in test_quantile_gpu.py): order statistics
equal a sort, quantiles equal torch.quantile bit for bit, sharded runs equal the single-process
run with no row gather and one all-reduce per radix pass."""
import json
import os

import numpy as np
import pytest
import torch

from harp_amd import cli
from harp_amd.models import stats as ST
from harp_amd.ops import quantile as QT
from harp_amd.runtime.launcher import launch
from harp_amd.utils import datasets as DS

from tests.test_reference_fixtures import P, rel

DTYPES = (torch.bfloat16, torch.float32, torch.float64)
NS = (1, 2, 255, 256, 257, 4097)
DS_ = (1, 3, 17, 65)
Q = (0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.999, 1)
KINDS = ("normal", "constant_column", "ties", "negative", "zeros", "inf", "denormal", "low_byte", "top_byte")
_INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}
_BITS = {torch.bfloat16: 16, torch.float32: 32, torch.float64: 64}


def block(kind: str, n: int, d: int, dtype: torch.dtype, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed * 1000003 + n * 131 + d)
    X = torch.randn(n, d, generator=g, dtype=torch.float64)
    if kind == "constant_column":
        X[:, d // 2] = 1.5
    elif kind == "ties":
        X = torch.randint(0, 4, (n, d), generator=g).double()
    elif kind == "negative":
        X = -X.abs() - 0.25
    elif kind == "zeros":  # +0.0, -0.0 and small values of both signs
        X = torch.where(torch.rand(n, d, generator=g) < 0.5, torch.zeros(()), X * 1e-3)
        X = torch.where(torch.rand(n, d, generator=g) < 0.3, -X, X)
    elif kind == "inf":
        X[torch.rand(n, d, generator=g) < 0.2] = float("inf")
        X[torch.rand(n, d, generator=g) < 0.2] = float("-inf")
    elif kind in ("denormal", "low_byte", "top_byte"):
        # built from bit patterns: denormals of both signs (exponent field 0); one value with
        # random low 8 key bits (only the last pass tells them apart); random top 8 bits over
        # fixed low bits (pass 0 decides), NaN patterns replaced
        w = _BITS[dtype]
        r = torch.randint(0, 256, (n, d), generator=g)
        if kind == "denormal":
            bits = (r & 63) + 1 + torch.where(r >= 128, -(1 << (w - 1)), 0)
        elif kind == "low_byte":
            bits = torch.full((n, d), 0x3F << (w - 8)) + r
        else:
            bits = (torch.where(r >= 128, r - 256, r) << (w - 8)) + 5
        X = bits.to(_INT[dtype]).view(dtype)
        return torch.where(torch.isnan(X), torch.ones((), dtype=dtype), X)
    return X.to(dtype)


def some_ranks(n: int):
    if n <= 257:
        return list(range(n))
    g = torch.Generator().manual_seed(n)
    return sorted(set([0, 1, n // 2, n - 2, n - 1] + torch.randint(0, n, (35,), generator=g).tolist()))


# ------------------------------------------------------------------ order statistics
@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32", "fp64"))
@pytest.mark.parametrize("kind", KINDS)
def test_order_statistics_equal_sort(kind, dtype):
    for n in NS:
        for d in DS_:
            X = block(kind, n, d, dtype)
            ranks = some_ranks(n)
            got = ST.order_statistics(X, ranks)
            assert got.dtype == dtype and got.shape == (len(ranks), d)
            assert torch.equal(got, torch.sort(X, 0).values[ranks]), (kind, n, d)


def test_test_blocks_are_what_they_claim():
    for dtype in DTYPES:
        w = _BITS[dtype]
        Z = block("zeros", 257, 3, dtype)
        assert bool(((Z == 0) & torch.signbit(Z)).any()) and bool(((Z == 0) & ~torch.signbit(Z)).any())
        D = block("denormal", 257, 3, dtype).double()
        assert bool((D != 0).all()) and float(D.abs().max()) < float(torch.finfo(dtype).tiny)
        lo = block("low_byte", 257, 3, dtype).view(_INT[dtype]).long()
        assert len(set((lo >> 8).reshape(-1).tolist())) == 1 and len(set(lo.reshape(-1).tolist())) > 100
        top = block("top_byte", 257, 3, dtype).view(_INT[dtype]).long()
        assert len(set((top & ((1 << (w - 8)) - 1)).reshape(-1).tolist())) <= 2


def test_strided_block_is_read_in_place():
    wide = block("normal", 300, 24, torch.float32)
    X = wide[:, 3:20]
    assert torch.equal(ST.order_statistics(X, [0, 150, 299]), torch.sort(X, 0).values[[0, 150, 299]])


def test_more_ranks_than_one_sweep():
    X = block("ties", 257, 5, torch.float32) + block("normal", 257, 5, torch.float32).round()
    ranks = list(range(0, 257, 12))
    assert QT.MAX_TARGETS >= 8 and QT.MAX_TARGETS < len(ranks) <= 3 * QT.MAX_TARGETS
    got = ST.order_statistics(X, ranks)
    one = torch.cat([ST.order_statistics(X, [r]) for r in ranks])
    assert torch.equal(got, one) and torch.equal(got, torch.sort(X, 0).values[ranks])


def test_bad_arguments():
    X = block("normal", 10, 2, torch.float32)
    with pytest.raises(ValueError, match="rank"):
        ST.order_statistics(X, [10])
    with pytest.raises(ValueError, match="no rows"):
        ST.order_statistics(X[:0], [0])
    with pytest.raises(ValueError, match="bf16, fp32 and fp64"):
        ST.order_statistics(X.half(), [0])
    with pytest.raises(ValueError, match="engine"):
        ST.quantiles(X, (0.5,), engine="hip")


# ------------------------------------------------------------------ quantiles
@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32", "fp64"))
@pytest.mark.parametrize("kind", ("normal", "ties", "constant_column", "zeros", "low_byte"))
def test_quantiles_equal_torch_quantile(kind, dtype):
    qt = torch.tensor(Q, dtype=torch.float64)
    for n in NS:
        for d in DS_:
            X = block(kind, n, d, dtype)
            got = ST.quantiles(X, Q, engine="native")
            assert got.dtype == torch.float64
            assert torch.equal(got, torch.quantile(X.double(), qt, dim=0)), (kind, n, d)


def test_quantiles_with_infinities_follow_torch():
    X = block("inf", 257, 17, torch.float32)
    ref = torch.quantile(X.double(), torch.tensor(Q, dtype=torch.float64), dim=0)  # inf - inf gives NaN there too
    assert torch.allclose(ST.quantiles(X, Q, engine="native"), ref, rtol=0, atol=0, equal_nan=True)


def test_default_engine_unchanged():
    X = block("normal", 100, 4, torch.float64)
    ref = torch.quantile(X, torch.tensor((0.1, 0.5, 0.9), dtype=torch.float64), dim=0)
    assert torch.equal(ST.quantiles(X), ref) and torch.equal(ST.quantiles(X, engine="torch"), ref)


def test_reference_fixture():
    X = DS.load_dense_csv(P("daal_quantile", "train", "quantiles.csv"))
    q = [0.1, 0.25, 0.5, 0.75, 0.9]
    got = ST.quantiles(X, q, engine="native").numpy()
    assert rel(got, np.quantile(X.numpy(), q, axis=0)) <= 1e-12


def test_nan_column():
    for dtype in DTYPES:
        X = block("normal", 300, 5, dtype)
        X[17, 2] = float("nan")
        X[250, 2] = float("nan")
        got = ST.quantiles(X, Q, engine="native")
        assert bool(got[:, 2].isnan().all()) and not bool(got[:, [0, 1, 3, 4]].isnan().any())
        ref = torch.quantile(X.double(), torch.tensor(Q, dtype=torch.float64), dim=0)
        assert torch.allclose(got, ref, rtol=0, atol=0, equal_nan=True)
        o = ST.order_statistics(X, [0, 299])
        assert bool(o[:, 2].isnan().all())
        keep = [0, 1, 3, 4]
        assert torch.equal(o[:, keep], torch.sort(X[:, keep], 0).values[[0, 299]])


def test_above_the_torch_limit():
    n = (1 << 24) + 1
    X = torch.randn(n, 1, generator=torch.Generator().manual_seed(5))
    with pytest.raises(ValueError, match='engine="native"'):
        ST.quantiles(X, (0.5,))
    got = ST.quantiles(X, (0.5,), engine="native")  # n is odd: the median is an element
    assert torch.equal(got, torch.sort(X, 0).values[n // 2].double()[None])


# ------------------------------------------------------------------ distributed
class _Hook:
    """Counts all-reduces; anything that gathers raises."""

    def __init__(self):
        self.allreduces = 0

    def __call__(self, op):
        if op == "all_reduce":
            self.allreduces += 1
        elif op != "barrier":
            raise AssertionError(f"collective {op} on the native quantile path")


def _boom(*a, **k):
    raise AssertionError("gather_rows on the native quantile path")


def _shard_worker(comm, shards, q):
    X = shards[comm.rank]
    hook = _Hook()
    saved = ST.gather_rows
    comm.fault_hook, ST.gather_rows = hook, _boom
    try:
        got = ST.quantiles(X, q, comm, engine="native")
    finally:
        comm.fault_hook, ST.gather_rows = None, saved
    return got, hook.allreduces


@pytest.mark.parametrize("world", (2, 3))
def test_sharded_equals_single_process(world):
    for dtype in DTYPES:
        X = block("ties", 401, 7, dtype) * 0.5 + block("normal", 401, 7, dtype).round()
        cuts = [0, 150, 150, 401] if world == 3 else [0, 401, 401]  # uneven, one shard empty
        shards = [X[cuts[r]:cuts[r + 1]] for r in range(world)]
        assert any(s.shape[0] == 0 for s in shards)
        ref = ST.quantiles(X, Q, engine="native")
        assert torch.equal(ref, torch.quantile(X.double(), torch.tensor(Q, dtype=torch.float64), dim=0))
        sweeps = -(-2 * len(Q) // QT.MAX_TARGETS)
        for got, allreduces in launch(_shard_worker, world, args=(shards, Q), timeout=300):
            assert torch.equal(got, ref)
            assert allreduces == QT.passes(dtype) * sweeps


def _empty_worker(comm, d):
    try:
        ST.quantiles(torch.zeros((0, d)), (0.5,), comm, engine="native")
    except ValueError as e:
        return str(e)
    return ""


def test_no_rows_anywhere_raises():
    assert all("no rows" in msg for msg in launch(_empty_worker, 2, args=(3,), timeout=300))


# ------------------------------------------------------------------ CLI
def test_cli_daal_quantile(tmp_path, capsys):
    X = block("normal", 90, 6, torch.float64).mul(100).round() / 100
    inp = tmp_path / "in"
    os.makedirs(inp)
    np.savetxt(inp / "block_1.csv", X[:35].numpy(), delimiter=",", fmt="%.17g")
    np.savetxt(inp / "block_2.csv", X[35:].numpy(), delimiter=",", fmt="%.17g")
    work = tmp_path / "out"
    assert cli.main(["daal", "quantile", "2", "1", "0", "1", str(inp), str(work), "--q", "0.1,0.5,0.75",
                     "--backend", "gloo"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["app"] == "daal"
    got = np.loadtxt(work / "quantile_quantiles.csv", delimiter=",")
    ref = ST.quantiles(X, (0.1, 0.5, 0.75), engine="native").numpy()
    assert got.shape == (3, 6) and np.array_equal(got, ref)
    assert cli.main(["daal", "qte", "2", "1", "0", "1", str(inp), str(tmp_path / "out2"), "--q", "0.1,0.5,0.75",
                     "--engine", "torch", "--backend", "gloo"]) == 0
    capsys.readouterr()
    assert np.array_equal(np.loadtxt(tmp_path / "out2" / "qte_quantiles.csv", delimiter=","), ref)
