"""Times the native optimization-solver engine (csrc/glm.hip) against the torch engine on one GPU:
(a) 1000 sgd steps at batch 4, d = 10 (the reference's setting) and (b) one value_grad at 10^7 x 32
in fp32 for MSE, logistic loss and cross-entropy with 16 classes. HIP events, 3 warm-ups, median of
10, the two engines alternating; one JSON line per measurement (profiles/optim/README.md)."""
import argparse
import json
import statistics

import torch

from harp_amd.models import optim as OP

HBM = 8e12  # bytes / s, the read floor's rate


def timed(fns, reps=10, warm=3):
    """Median milliseconds of every callable, the callables alternating inside each repetition."""
    for _ in range(warm):
        for f in fns:
            f()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [statistics.median(m) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 7)
    ap.add_argument("--out", default="bench_optim.jsonl")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_optim.py needs a GPU"
    dev, g = torch.device("cuda", 0), torch.Generator().manual_seed(0)
    lines = []

    # (a) the reference's stochastic setting
    X = torch.randn(10000, 10, generator=g).to(dev)
    y = (X.double().sum(1) + 0.5).contiguous()
    for kind, cls in (("mse", OP.MSE), ("logistic", OP.LogisticLoss)):
        yk = y if kind == "mse" else (y > 0).double()
        objs = [cls(X, yk, engine=e) for e in ("native", "torch")]
        run = lambda o: OP.sgd(o, None, 1000, 0.01, 4, seed=1)  # noqa: E731
        nat, ref = timed([lambda: run(objs[0]), lambda: run(objs[1])], reps=10, warm=1)
        diff = float((run(objs[0]).minimum - run(objs[1]).minimum).abs().max())
        lines.append(dict(what="sgd 1000 steps, batch 4, d 10", kind=kind, native_ms=nat, torch_ms=ref, max_diff=diff))

    # (b) one full-block value_grad
    n, d, K = a.rows, 32, 16
    X = torch.randn(n, d, generator=g).to(dev)
    z = X[:, 0].double()
    floor = X.numel() * X.element_size() / HBM * 1e3
    cases = (("mse", lambda e: OP.MSE(X, z + 0.5, engine=e)),
             ("logistic", lambda e: OP.LogisticLoss(X, (z > 0).double(), engine=e)),
             ("cross_entropy", lambda e: OP.CrossEntropyLoss(X, (z.abs() * 5).long().clamp_(0, K - 1), K, engine=e)))
    for kind, make in cases:
        objs = [make("native"), make("torch")]
        x = torch.randn(objs[0].dim, generator=g, dtype=torch.float64).to(dev) * 0.1
        nat, ref = timed([lambda: objs[0].value_grad(x), lambda: objs[1].value_grad(x)])
        gn, gt = objs[0].value_grad(x)[1], objs[1].value_grad(x)[1]
        lines.append(dict(what=f"value_grad {n} x {d} fp32", kind=kind, native_ms=nat, torch_ms=ref, floor_ms=floor,
                          native_over_floor=nat / floor, max_diff=float((gn - gt).abs().max())))
    with open(a.out, "w") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
