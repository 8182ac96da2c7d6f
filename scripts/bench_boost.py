"""Boosting engines on one GPU: ``engine="native"`` (csrc/boost.hip) against ``engine="torch"``
in the same process on the same data, ``fit`` and ``predict``.

Timing: hipEvents around each call, ``--warmup`` untimed calls, then the median of ``--runs``
timed ones with the spread (min .. max); the torch engine takes ``--torch-warmup`` /
``--torch-runs``. One more native fit per algorithm is instrumented per round (events around
the round kernel, the split kernels and the scalar updates; the host read is timed on the wall
clock after a synchronize, so it is the read alone). The fused class round is compared with an
unfused A/B in the same binary (update pass, then a histogram-only pass).

    python scripts/bench_boost.py --algo adaboost     # 1e6 x 32, 3 classes, 256 bins, 50 rounds
    python scripts/bench_boost.py --algo logitboost   # same rows, K = 5, 20 rounds
    python scripts/bench_boost.py --algo brownboost   # same rows, 2 classes, 40 rounds
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harp_amd.models import trees as T  # noqa: E402
from harp_amd.ops import boost as BO  # noqa: E402
from harp_amd.ops import forest as F  # noqa: E402

ALGOS = {"adaboost": dict(C=3, rounds=50), "logitboost": dict(C=5, rounds=20), "brownboost": dict(C=2, rounds=40)}


def make_data(n, d, C, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    X = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32)
    s = X[:, 0] * 1.5 + X[:, d // 2] * X[:, d - 1].sign() + 0.4 * torch.randn(n, generator=g, device=dev)
    q = torch.quantile(s[:200000].double(), torch.linspace(0, 1, C + 1, dtype=torch.float64, device=dev)[1:-1])
    return X, torch.bucketize(s.double(), q)


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms)}


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return spread(ms)


class Marks:
    """Event pairs per stage; ``ms()`` after a synchronize."""

    def __init__(self):
        self.pairs = []

    def __call__(self, stage, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self.pairs.append((stage, e0, e1))
        return out

    def ms(self, rounds):
        torch.cuda.synchronize()
        tot = {}
        for stage, e0, e1 in self.pairs:
            tot[stage] = tot.get(stage, 0.0) + e0.elapsed_time(e1)
        return {k: v / rounds for k, v in tot.items()}


def ada_round_split(Xb, y, d, B, C, rounds):
    """Per-round milliseconds of the stages of ``ops.boost.ada_fit`` (the same calls)."""
    n = Xb.shape[0]
    w = [torch.ones(n, dtype=torch.float64, device=Xb.device), torch.empty(n, dtype=torch.float64, device=Xb.device)]
    rec, mul = BO.new_class_state(Xb.device)
    mk, read = Marks(), []
    for t in range(rounds):
        H = mk("round_kernel", lambda: BO.class_round(Xb, y, w[t & 1], w[(t + 1) & 1], rec, mul, d, B, C))
        bf, bb, _, sp, L, R, Tt = mk("split_kernels", lambda: BO.root_split(H, F.GINI))
        info = mk("scalar_updates", lambda: BO.class_finish(bf, bb, sp, L, R, Tt, float(n), rec, mul))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info.tolist()
        read.append((time.perf_counter() - t0) * 1e3)
    out = mk.ms(rounds)
    out["host_read"] = statistics.median(read)
    return out, (rec, mul, w[rounds & 1])


def logit_round_split(Xb, y, d, B, K, rounds):
    n = Xb.shape[0]
    Fb = [torch.zeros((n, K), dtype=torch.float64, device=Xb.device),
          torch.empty((n, K), dtype=torch.float64, device=Xb.device)]
    rec_i, rec_v = BO.new_logit_state(K, Xb.device)
    mk = Marks()
    for t in range(rounds):
        ri, rv = rec_i, rec_v
        H = mk("round_kernel", lambda: BO.logit_round(Xb, y, Fb[t & 1], Fb[(t + 1) & 1], ri, rv, 4.0, d, B, K))
        bf, bb, _, sp, L, R, Tt = mk("split_kernels", lambda: BO.root_split(H, F.MSE))
        rec_i, rec_v, _ = mk("scalar_updates", lambda: BO.logit_records(bf, bb, sp, L, R, Tt))
    out = mk.ms(rounds)
    out["host_read"] = 0.0  # none per round: one read per fit
    return out


def fused_ab(Xb, y, d, B, C, state, warmup, runs):
    """The fused round against update pass + histogram-only pass, on a real stump state."""
    rec, mul, w = state
    n = Xb.shape[0]
    none, one = BO.new_class_state(Xb.device)
    w1, w2 = torch.empty_like(w), torch.empty_like(w)

    def unfused():
        BO.class_update(Xb, y, w, w1, rec, mul, d)
        BO.class_round(Xb, y, w1, w2, none, one, d, B, C)

    return {"fused": timed(lambda: BO.class_round(Xb, y, w, w1, rec, mul, d, B, C), warmup, runs),
            "unfused": timed(unfused, warmup, runs),
            "hist_only": timed(lambda: BO.class_round(Xb, y, w1, w2, none, one, d, B, C), warmup, runs)}


def torch_brown_reads(fit):
    """Host reads of the torch engine's line search: every potential it evaluates is read."""
    calls, erf = [0], torch.erf
    torch.erf = lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), erf(*a, **k))[1]
    try:
        m = fit()
    finally:
        torch.erf = erf
    return calls[0] / max(len(m.learners), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algo", choices=sorted(ALGOS), default="adaboost")
    ap.add_argument("--n", type=int, default=10 ** 6)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=0)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-runs", type=int, default=None)
    ap.add_argument("--torch-warmup", type=int, default=None)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sh = dict(ALGOS[a.algo], n=a.n, d=a.d, B=256)
    if a.rounds:
        sh["rounds"] = a.rounds
    n, d, C, B, rounds = sh["n"], sh["d"], sh["C"], sh["B"], sh["rounds"]
    dev = torch.device("cuda", 0)
    X, y = make_data(n, d, C, dev)
    res = {"algo": a.algo, "shape": sh, "device": torch.cuda.get_device_name(0)}

    def model(engine):
        if a.algo == "adaboost":
            return T.AdaBoost(rounds, engine=engine)
        if a.algo == "logitboost":
            return T.LogitBoost(rounds, engine=engine)
        return T.BrownBoost(c=2.0, max_rounds=rounds, engine=engine)

    fitted = {}

    def fit(engine):
        fitted[engine] = model(engine).fit(X, y)
        return fitted[engine]

    for engine in ["native"] + ([] if a.skip_torch else ["torch"]):
        native = engine == "native"
        runs = a.runs if native or a.torch_runs is None else a.torch_runs
        warm = a.warmup if native or a.torch_warmup is None else a.torch_warmup
        res[engine + "_fit"] = timed(lambda: fit(engine), warm, runs)
        res[engine + "_predict"] = timed(lambda: fitted[engine].predict(X), warm, runs)
        res[engine + "_train_acc"] = float((fitted[engine].predict(X) == y).double().mean())
        m = fitted[engine]
        res[engine + "_learners"] = len(m.rounds) if a.algo == "logitboost" else len(m.learners)
        print(json.dumps({k: v for k, v in res.items() if k.startswith(engine)}), flush=True)

    th = T._bins(X, B)
    res["quantiles"] = timed(lambda: T._bins(X, B), 1, 3)
    res["binning"] = timed(lambda: F.bin_features(X, th), 1, 3)
    Xb, yi = F.bin_features(X, th), y.int()
    if a.algo == "logitboost":
        res["round_ms"] = logit_round_split(Xb, yi, d, B, C, rounds)
    else:
        res["round_ms"], state = ada_round_split(Xb, yi, d, B, C, min(rounds, 10))
        res["fused_ab"] = fused_ab(Xb, yi, d, B, C, state, a.warmup, a.runs)
    if a.algo == "brownboost":
        res["native_host_reads_per_round"] = statistics.mean(fitted["native"].host_reads)
        if not a.skip_torch:
            res["torch_host_reads_per_round"] = torch_brown_reads(lambda: fit("torch"))
    res["round_read_floor_ms"] = n * (F.padded_width(d) + 12) / 4.0e12 * 1e3  # bytes of the round at ~4 TB/s
    res["lds_adds_per_round"] = n * d * (3 * C if a.algo == "logitboost" else 1)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
