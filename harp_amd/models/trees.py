"""Decision trees, decision forests and boosting.

Reference: ml/daal batch algorithms ``daal_dtree`` (classification / regression, plus
"traverse" variants that walk the trained model), ``daal_dforest`` (classification /
regression forests), ``daal_stump``, ``daal_adaboost``, ``daal_brownboost``,
``daal_logitboost``; contrib random forests (contrib/.../randomforest, rf, com/rf/fast:
per-mapper trees on local data, predictions combined by vote through allreduce / reduce).

Trees grow level-wise with histogram split search: features are quantile-binned once, then
per level (node, feature, bin) histograms of the class counts (or weight / target sums) are
built, a prefix sum over bins scores every candidate split and the samples are re-routed.
Two engines train the same ``DecisionTree`` arrays (``feature / threshold / left / value``,
children numbered in level order, left then right):

* ``engine="torch"`` (default) — plain torch, one tree at a time: per level one fp64
  ``index_add_`` over an expanded [n, d, C] value tensor builds the histograms, a host loop
  over the frontier nodes (``.item()`` reads, ``randperm`` feature subsets) picks the splits,
  and prediction gathers once per depth and tree. It runs anywhere torch does.
* ``engine="native"`` — ``ops/forest.py`` + ``csrc/forest.hip``: all trees of a batch grow
  together with the tree arrays on the device and one host read per level; uint8 bins,
  counter-based bootstrap multiplicities and hashed feature subsets, LDS histograms (exact
  integer counts for classification with integer multiplicities, fp64 sums otherwise), a
  wave per (node, feature) split search and a packed-forest prediction kernel. HIP tensors
  run the kernels, CPU tensors the torch mirror of the same algorithm. ``DecisionForest`` can
  then also train one model over row shards (``fit_distributed(mode="rows")``: one histogram
  all-reduce per level).

The boosting classes (``stump``, ``AdaBoost``, ``LogitBoost``, ``BrownBoost``) take the same
``engine`` argument. ``"torch"`` (default) fits a fresh ``DecisionTree`` per learner.
``"native"`` — ``ops/boost.py`` + ``csrc/boost.hip`` — bins the features once per fit and runs
one fused pass over the binned rows per round (the previous learner's weight or
working-response update plus the root histogram), then the forest engine's split kernels;
BrownBoost's search for the time step runs on the device. The learners are ordinary
``DecisionTree`` objects, so models of the two engines are interchangeable, and
``AdaBoost`` / ``LogitBoost`` can train one model over row shards (``fit_distributed``: one
histogram all-reduce per round). On HIP tensors their ``decision`` walks all stumps in the
packed-forest prediction kernel.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from ..core.writable import DataInput, DataOutput, Writable
from ..ops import boost as BO
from ..ops import forest as F
from ..parallel.comm import Communicator

ENGINES = ("torch", "native")


def _n_sub(max_features, d: int) -> Optional[int]:
    """Features per node of the native engine (None = all), the torch engine's rule."""
    if not max_features:
        return None
    return max_features if isinstance(max_features, int) else max(1, int(math.sqrt(d)))


def _trees_from_packed(packed: dict, th: torch.Tensor, proto: "DecisionTree", seeds) -> List["DecisionTree"]:
    """DecisionTree objects (CPU arrays, as the torch engine leaves them) from ``ops.forest.grow``."""
    f = packed["feature"]
    thr = torch.where(f >= 0, th.to(f.device)[f.clamp_min(0), packed["bin"]], torch.zeros((), dtype=torch.float64,
                                                                                          device=f.device))
    V = packed["stats"]
    if proto.task == "classification":
        val = V / V.sum(1, keepdim=True).clamp_min(1e-300)
    else:
        val = (V[:, 1] / V[:, 0].clamp_min(1e-300))[:, None]
    f, thr, left, val = f.cpu(), thr.cpu(), packed["left"].cpu(), val.cpu()
    out, a = [], 0
    for size, seed in zip(packed["sizes"], seeds):
        t = DecisionTree(proto.task, proto.max_depth, proto.min_leaf, proto.max_features, proto.n_bins,
                         proto.criterion, seed=seed, engine="native")
        t.feature, t.threshold, t.left, t.value = f[a:a + size], thr[a:a + size], left[a:a + size], val[a:a + size]
        out.append(t)
        a += size
    return out


def _bins(X: torch.Tensor, n_bins: int) -> torch.Tensor:
    """Per-feature quantile thresholds [d, n_bins-1]."""
    q = torch.linspace(0, 1, n_bins + 1, dtype=torch.float64, device=X.device)[1:-1]
    Xs = X.double()
    if Xs.shape[0] > 200000:
        idx = torch.randint(0, Xs.shape[0], (200000,), device=X.device)
        Xs = Xs[idx]
    return torch.quantile(Xs, q, dim=0).t().contiguous()


class DecisionTree(Writable):
    """CART tree. ``task``: "classification" (gini / entropy) or "regression" (mse)."""

    def __init__(self, task: str = "classification", max_depth: int = 8, min_samples_leaf: int = 1,
                 max_features=None, n_bins: int = 64, criterion: str = "gini", seed: int = 0,
                 engine: str = "torch"):
        if engine not in ENGINES:
            raise ValueError(f"engine must be one of {ENGINES} (got {engine!r})")
        self.engine = engine
        self.task, self.max_depth, self.min_leaf = task, max_depth, min_samples_leaf
        self.max_features, self.n_bins, self.criterion, self.seed = max_features, n_bins, criterion, seed
        self.feature = torch.empty(0, dtype=torch.int64)
        self.threshold = torch.empty(0, dtype=torch.float64)
        self.left = torch.empty(0, dtype=torch.int64)
        self.value = torch.empty(0, 0, dtype=torch.float64)

    # ---------------------------------------------------------------- training
    def fit(self, X: torch.Tensor, y: torch.Tensor, sample_weight: Optional[torch.Tensor] = None,
            num_classes: Optional[int] = None, thresholds: Optional[torch.Tensor] = None) -> "DecisionTree":
        if self.engine == "native":
            return self._fit_native(X, y, sample_weight, num_classes, thresholds)
        dev = X.device
        n, d = X.shape
        w = torch.ones(n, dtype=torch.float64, device=dev) if sample_weight is None else sample_weight.double().to(dev)
        cls = self.task == "classification"
        if cls:
            C = int(num_classes or int(y.max()) + 1)
            stats = torch.nn.functional.one_hot(y.long().to(dev), C).double() * w[:, None]
        else:
            yd = y.double().to(dev).reshape(n)
            stats = torch.stack([w, w * yd, w * yd * yd], 1)
            C = 3
        th = thresholds if thresholds is not None else _bins(X, self.n_bins)
        B = th.shape[1] + 1
        Xb = torch.searchsorted(th, X.double().t().contiguous(), right=True).t()  # [n, d] bin ids
        gen = torch.Generator(device="cpu").manual_seed(self.seed)
        feats, thrs, lefts, vals = [], [], [], []
        node_of = torch.zeros(n, dtype=torch.int64, device=dev)
        frontier = [0]
        feats.append(-1), thrs.append(0.0), lefts.append(-1)
        vals.append(stats.sum(0))
        depth = 0
        while frontier and depth < self.max_depth:
            m = len(frontier)
            fmap = torch.full((len(feats),), -1, dtype=torch.int64, device=dev)
            fmap[torch.tensor(frontier, device=dev)] = torch.arange(m, device=dev)
            loc = fmap[node_of]
            act = loc >= 0
            if not bool(act.any()):
                break
            li, lx, ls = loc[act], Xb[act], stats[act]
            # histogram [m, d, B, C]
            H = torch.zeros((m * d * B, C), dtype=torch.float64, device=dev)
            idx = (li[:, None] * d + torch.arange(d, device=dev)[None, :]) * B + lx
            H.index_add_(0, idx.reshape(-1), ls[:, None, :].expand(-1, d, -1).reshape(-1, C))
            H = H.view(m, d, B, C)
            Lc = H.cumsum(2)[:, :, :-1, :]  # left = bins <= b
            tot = H.sum(2, keepdim=True)
            Rc = tot - Lc
            gain = self._gain(Lc, Rc, tot)
            # feature subsampling
            if self.max_features:
                k = self.max_features if isinstance(self.max_features, int) else max(1, int(math.sqrt(d)))
                mask = torch.full((m, d), float("-inf"), dtype=torch.float64, device=dev)
                for j in range(m):
                    sel = torch.randperm(d, generator=gen)[:k].to(dev)
                    mask[j, sel] = 0.0
                gain = gain + mask[:, :, None]
            nL = self._count(Lc)
            nR = self._count(Rc)
            gain = torch.where((nL >= self.min_leaf) & (nR >= self.min_leaf), gain, torch.full_like(gain, float("-inf")))
            flat = gain.reshape(m, -1)
            best, arg = flat.max(1)
            bf, bb = arg // (B - 1), arg % (B - 1)
            new_frontier = []
            split_nodes = []
            for j, node in enumerate(frontier):
                if best[j].item() > 1e-12:
                    f, b = int(bf[j]), int(bb[j])
                    feats[node], thrs[node] = f, float(th[f, b])
                    lefts[node] = len(feats)
                    for side in (Lc, Rc):
                        feats.append(-1), thrs.append(0.0), lefts.append(-1)
                        vals.append(side[j, f, b])
                    new_frontier += [lefts[node], lefts[node] + 1]
                    split_nodes.append((node, f, b))
            if not split_nodes:
                break
            # route samples of split nodes
            feat_t = torch.tensor(feats, device=dev)
            bin_t = torch.full((len(feats),), 0, dtype=torch.int64, device=dev)
            for node, f, b in split_nodes:
                bin_t[node] = b
            left_t = torch.tensor(lefts, device=dev)
            is_split = left_t[node_of] >= 0
            fsel = feat_t[node_of].clamp_min(0)
            go_right = Xb.gather(1, fsel[:, None])[:, 0] > bin_t[node_of]
            node_of = torch.where(is_split, left_t[node_of] + go_right.long(), node_of)
            frontier = new_frontier
            depth += 1
        self.feature = torch.tensor(feats, dtype=torch.int64)
        self.threshold = torch.tensor(thrs, dtype=torch.float64)
        self.left = torch.tensor(lefts, dtype=torch.int64)
        V = torch.stack(vals).cpu()
        if cls:
            self.value = V / V.sum(1, keepdim=True).clamp_min(1e-300)
        else:
            self.value = (V[:, 1] / V[:, 0].clamp_min(1e-300))[:, None]
        return self

    def _fit_native(self, X, y, sample_weight, num_classes, thresholds) -> "DecisionTree":
        """One tree through ``ops.forest.grow``. Statistics kind: classification without
        weights or with integer weights (<= 255) -> exact integer counts; real weights and
        regression -> fp64 sums."""
        dev = X.device
        n, d = X.shape
        cls = self.task == "classification"
        C = int(num_classes or int(y.max()) + 1) if cls else 3
        th = thresholds if thresholds is not None else _bins(X, self.n_bins)
        B = th.shape[1] + 1
        F.check_shape(B, C)
        w = None if sample_weight is None else sample_weight.to(dev)
        integer = w is None or bool(((w == w.round()) & (w >= 0) & (w <= 255)).all())
        if integer and w is not None and float(w.sum()) >= 2.0 ** 32:
            integer = False
        mult = torch.ones((1, n), dtype=torch.uint8, device=dev)
        yi = stats = None
        if cls and integer:
            kind = F.COUNT
            yi = y.to(dev).int()
            if w is not None:
                mult = w.to(torch.uint8).reshape(1, n)
        else:
            kind = F.REAL
            wd = torch.ones(n, dtype=torch.float64, device=dev) if w is None else w.double()
            if cls:
                stats = torch.nn.functional.one_hot(y.long().to(dev), C).double() * wd[:, None]
            else:
                yd = y.double().to(dev).reshape(n)
                stats = torch.stack([wd, wd * yd, wd * yd * yd], 1)
        packed = F.grow(F.bin_features(X, th), d, B, C, kind, mult, task=F.task_id(self.task, self.criterion),
                        max_depth=self.max_depth, min_leaf=self.min_leaf, k_sub=_n_sub(self.max_features, d),
                        seed=self.seed, y=yi, stats=stats)
        t = _trees_from_packed(packed, th, self, [self.seed])[0]
        self.feature, self.threshold, self.left, self.value = t.feature, t.threshold, t.left, t.value
        return self

    def _count(self, S):
        return S.sum(-1) if self.task == "classification" else S[..., 0]

    def _impurity(self, S):
        if self.task == "classification":
            n = S.sum(-1, keepdim=True).clamp_min(1e-300)
            p = S / n
            if self.criterion == "entropy":
                return -(p * torch.log2(p.clamp_min(1e-300))).sum(-1) * n[..., 0]
            return (1 - (p * p).sum(-1)) * n[..., 0]
        w, s, ss = S[..., 0], S[..., 1], S[..., 2]
        return ss - s * s / w.clamp_min(1e-300)

    def _gain(self, L, R, T):
        return self._impurity(T) - self._impurity(L) - self._impurity(R)

    # ---------------------------------------------------------------- inference
    def apply(self, X: torch.Tensor) -> torch.Tensor:
        """Leaf index of every sample (the DAAL "traverse" variants walk the same arrays)."""
        dev = X.device
        f, t, l = self.feature.to(dev), self.threshold.to(dev), self.left.to(dev)
        node = torch.zeros(X.shape[0], dtype=torch.int64, device=dev)
        Xd = X.double()
        for _ in range(self.max_depth + 1):
            lf = l[node]
            inner = lf >= 0
            if not bool(inner.any()):
                break
            xv = Xd.gather(1, f[node].clamp_min(0)[:, None])[:, 0]
            node = torch.where(inner, lf + (xv >= t[node]).long(), node)  # training: left <=> x < thr
        return node

    def predict_proba(self, X: torch.Tensor) -> torch.Tensor:
        return self.value.to(X.device)[self.apply(X)]

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        v = self.predict_proba(X)
        return v.argmax(1) if self.task == "classification" else v[:, 0]

    # ---------------------------------------------------------------- wire format
    def write(self, out: DataOutput) -> None:
        out.write_utf(self.task)
        out.write_int(self.max_depth)
        out.write_int(self.feature.numel())
        out.write_int(self.value.shape[1])
        for i in range(self.feature.numel()):
            out.write_int(int(self.feature[i]))
            out.write_double(float(self.threshold[i]))
            out.write_int(int(self.left[i]))
            for v in self.value[i].tolist():
                out.write_double(v)

    def read(self, inp: DataInput) -> None:
        self.task = inp.read_utf()
        self.max_depth = inp.read_int()
        n, c = inp.read_int(), inp.read_int()
        f, t, l, v = [], [], [], []
        for _ in range(n):
            f.append(inp.read_int())
            t.append(inp.read_double())
            l.append(inp.read_int())
            v.append([inp.read_double() for _ in range(c)])
        self.feature = torch.tensor(f, dtype=torch.int64)
        self.threshold = torch.tensor(t, dtype=torch.float64)
        self.left = torch.tensor(l, dtype=torch.int64)
        self.value = torch.tensor(v, dtype=torch.float64).reshape(n, c)


class DecisionForest:
    """Random forest: bootstrap rows + sqrt(d) features per split. ``fit_distributed``
    trains ``n_trees / P`` trees per worker on its local rows and all-gathers the trees
    (the contrib RF combines per-mapper trees the same way); with ``engine="native"`` and
    ``mode="rows"`` it trains ONE forest over the workers' row shards instead (Poisson(1)
    bootstrap keyed by the global row index, one histogram all-reduce per level)."""

    def __init__(self, task="classification", n_trees=50, max_depth=10, max_features="sqrt", n_bins=64, seed=0,
                 min_samples_leaf=1, engine="torch", criterion="gini"):
        if engine not in ENGINES:
            raise ValueError(f"engine must be one of {ENGINES} (got {engine!r})")
        self.engine, self.criterion = engine, criterion
        self._pack = None
        self.task, self.n_trees, self.max_depth = task, n_trees, max_depth
        self.max_features, self.n_bins, self.seed, self.min_leaf = max_features, n_bins, seed, min_samples_leaf
        self.trees: List[DecisionTree] = []
        self.num_classes = None

    def fit(self, X, y, num_classes=None, n_trees=None, seed_offset=0, thresholds=None):
        n = X.shape[0]
        self.num_classes = num_classes or (int(y.max()) + 1 if self.task == "classification" else None)
        th = thresholds if thresholds is not None else _bins(X, self.n_bins)
        if self.engine == "native":
            return self._fit_native(X, y, th, n_trees or self.n_trees, self.seed + seed_offset)
        g = torch.Generator().manual_seed(self.seed + seed_offset)
        for t in range(n_trees or self.n_trees):
            idx = torch.randint(0, n, (n,), generator=g).to(X.device)
            w = torch.bincount(idx, minlength=n).double()
            tree = DecisionTree(self.task, self.max_depth, self.min_leaf, self.max_features, self.n_bins,
                                self.criterion, seed=self.seed * 1000 + seed_offset + t)
            self.trees.append(tree.fit(X, y, sample_weight=w, num_classes=self.num_classes, thresholds=th))
        return self

    def _fit_native(self, X, y, th, n_trees, seed, row0=0, reduce=None, n_total=None):
        """Train ``n_trees`` trees in batches through ``ops.forest.grow`` and append them.
        ``n_total``: rows over all shards (the batch size must not depend on the shard)."""
        dev = X.device
        n, d = X.shape
        cls = self.task == "classification"
        C = int(self.num_classes) if cls else 3
        B = th.shape[1] + 1
        F.check_shape(B, C)
        Xb = F.bin_features(X, th)
        yi = stats = None
        if cls:
            kind, yi = F.COUNT, y.to(dev).int()
        else:
            kind = F.REAL
            yd = y.double().to(dev).reshape(n)
            stats = torch.stack([torch.ones_like(yd), yd, yd * yd], 1)
        proto = DecisionTree(self.task, self.max_depth, self.min_leaf, self.max_features, self.n_bins,
                             self.criterion, engine="native")
        step = F.trees_per_batch(n_total or n, d, B, C, kind, self.max_depth)
        for t0 in range(0, n_trees, step):
            tb = min(step, n_trees - t0)
            mult = F.bootstrap(seed, t0, tb, row0, n, dev)
            packed = F.grow(Xb, d, B, C, kind, mult, task=F.task_id(self.task, self.criterion),
                            max_depth=self.max_depth,
                            min_leaf=self.min_leaf, k_sub=_n_sub(self.max_features, d), seed=seed, tree0=t0, y=yi,
                            stats=stats, reduce=reduce)
            self.trees += _trees_from_packed(packed, th, proto, [seed * 1000 + t0 + i for i in range(tb)])
        self._pack = None
        return self

    def _fit_rows(self, X, y, comm: Communicator, num_classes, thresholds):
        """Data-parallel fit: every worker holds a row shard and ends with the same forest."""
        if self.engine != "native":
            raise ValueError('fit_distributed(mode="rows") needs engine="native"')
        sizes = comm.all_gather_ints([X.shape[0]])[:, 0].tolist()
        row0 = sum(sizes[:comm.rank])
        if self.task == "classification":
            if num_classes is None:
                top = torch.tensor([int(y.max()) if y.numel() else 0], dtype=torch.int64, device=comm.device)
                comm.all_reduce(top, op=torch.distributed.ReduceOp.MAX)
                num_classes = int(top) + 1
            self.num_classes = int(num_classes)
        th = thresholds
        if th is None:  # rank 0's quantiles for everyone
            th = _bins(X, self.n_bins) if comm.rank == 0 else torch.empty((X.shape[1], self.n_bins - 1),
                                                                          dtype=torch.float64, device=X.device)
            th = th.contiguous()
            comm.broadcast(th, 0)
        return self._fit_native(X, y, th.to(X.device), self.n_trees, self.seed, row0=row0,
                                reduce=lambda H: comm.all_reduce(H), n_total=sum(sizes))

    def fit_distributed(self, X, y, comm: Communicator, num_classes=None, mode="trees", thresholds=None):
        """``mode="trees"``: whole trees per worker on its local rows, all-gathered.
        ``mode="rows"`` (native engine): one forest over the workers' row shards."""
        from ..parallel.partition_util import allgather_objects

        if mode == "rows":
            return self._fit_rows(X, y, comm, num_classes, thresholds)
        if mode != "trees":
            raise ValueError(f'mode must be "trees" or "rows" (got {mode!r})')
        P, r = comm.world_size, comm.rank
        mine = self.n_trees // P + (1 if r < self.n_trees % P else 0)
        self.fit(X, y, num_classes, n_trees=mine, seed_offset=7919 * r)
        self.trees = allgather_objects(comm, self.trees)
        self._pack = None
        return self

    def _packed(self, device):
        """The forest's arrays concatenated on ``device`` (built once per forest and device)."""
        key = (str(device), len(self.trees))
        if self._pack is None or self._pack[0] != key:
            self._pack = (key, F.pack_trees(self.trees, device))
        return self._pack[1]

    def _use_kernel(self, X) -> bool:
        return self.engine == "native" and X.device.type == "cuda" and len(self.trees) > 0

    def apply(self, X):
        """Leaf index of every sample in every tree, [n_trees, n]."""
        if self._use_kernel(X):
            return F.predict_packed(X, self._packed(X.device), proba=False, leaves=True)[1]
        return torch.stack([t.apply(X) for t in self.trees])

    def predict_proba(self, X):
        if self._use_kernel(X):
            return F.predict_packed(X, self._packed(X.device))[0]
        return torch.stack([t.predict_proba(X) for t in self.trees]).mean(0)

    def predict(self, X):
        p = self.predict_proba(X)
        return p.argmax(1) if self.task == "classification" else p[:, 0]


# ---------------------------------------------------------------- boosting
def _check_engine(engine: str) -> str:
    if engine not in ENGINES:
        raise ValueError(f"engine must be one of {ENGINES} (got {engine!r})")
    return engine


def _stump_tree(task: str, n_bins: int, split: bool, feature: int, threshold: float, values) -> DecisionTree:
    """A depth-1 ``DecisionTree`` from (root, left, right) node values [3, C]; a bare root if
    ``split`` is false."""
    t = DecisionTree(task, max_depth=1, n_bins=n_bins, engine="native")
    m = 3 if split else 1
    t.feature = torch.tensor([feature if split else -1, -1, -1][:m], dtype=torch.int64)
    t.threshold = torch.tensor([threshold if split else 0.0, 0.0, 0.0][:m], dtype=torch.float64)
    t.left = torch.tensor([1 if split else -1, -1, -1][:m], dtype=torch.int64)
    t.value = torch.as_tensor(values, dtype=torch.float64)[:m].reshape(m, -1)
    return t


def _class_stump(info, th: torch.Tensor, C: int) -> DecisionTree:
    """Classification stump from a ``ops.boost.class_finish`` record (``th`` on the CPU)."""
    f, b = int(info[1]), int(info[2])
    L = torch.tensor(info[BO.INFO:BO.INFO + C], dtype=torch.float64)
    R = torch.tensor(info[BO.INFO + C:BO.INFO + 2 * C], dtype=torch.float64)
    V = torch.stack([L + R, L, R])
    V = V / V.sum(1, keepdim=True).clamp_min(1e-300)
    return _stump_tree("classification", th.shape[1] + 1, bool(info[0]), f, float(th[f, b]), V)


def _shards(X, y, comm: Communicator, num_classes, thresholds, n_bins: int):
    """What the workers of a row-sharded fit agree on first: (classes, thresholds, total rows).
    Rank 0's quantiles serve everyone, as in ``DecisionForest._fit_rows``."""
    n_total = int(comm.all_gather_ints([X.shape[0]])[:, 0].sum())
    if num_classes is None:
        top = torch.tensor([int(y.max()) if y.numel() else 0], dtype=torch.int64, device=comm.device)
        comm.all_reduce(top, op=torch.distributed.ReduceOp.MAX)
        num_classes = int(top) + 1
    th = thresholds
    if th is None:
        th = _bins(X, n_bins) if comm.rank == 0 else torch.empty((X.shape[1], n_bins - 1), dtype=torch.float64,
                                                                 device=X.device)
        th = th.contiguous()
        comm.broadcast(th, 0)
    return int(num_classes), th.to(X.device), n_total


def _packed_sum(X, trees, values, K: int, cache: dict):
    """Sum over ``trees`` of their leaf rows in ``values`` (one [nodes, K] tensor per tree)
    through the packed-forest prediction kernel, [n, K] fp64. ``cache`` keeps the pack while
    the device and the tree arrays stay the same objects and ``values`` compare equal."""
    arrays = [a for t in trees for a in (t.feature, t.threshold, t.left, t.value)]
    hit = (cache.get("device") == str(X.device) and len(cache["arrays"]) == len(arrays)
           and all(a is b for a, b in zip(cache["arrays"], arrays))
           and all(torch.equal(a, b) for a, b in zip(cache["values"], values)))
    if not hit:
        from types import SimpleNamespace

        cache["device"], cache["arrays"], cache["values"] = str(X.device), arrays, values
        cache["pack"] = F.pack_trees([SimpleNamespace(feature=t.feature, threshold=t.threshold, left=t.left, value=v)
                                      for t, v in zip(trees, values)], X.device)
    return F.predict_packed(X, cache["pack"])[0] * len(trees)


def stump(X, y, sample_weight=None, num_classes=None, task="classification", engine="torch"):
    """Decision stump (daal_stump): a depth-1 tree. ``engine="native"`` (classification): one
    round of ``ops.boost`` with the weights scaled to sum n."""
    if _check_engine(engine) == "torch":
        return DecisionTree(task, max_depth=1, n_bins=256).fit(X, y, sample_weight, num_classes)
    if task != "classification":
        return DecisionTree(task, max_depth=1, n_bins=256, engine="native").fit(X, y, sample_weight, num_classes)
    n, d = X.shape
    C = int(num_classes or int(y.max()) + 1)
    F.check_shape(256, C)
    th = _bins(X, 256)
    w0 = None if sample_weight is None else sample_weight.double().to(X.device) * (n / float(sample_weight.sum()))
    got = []
    BO.ada_fit(F.bin_features(X, th), y.to(X.device), d, 256, C, 1, w0=w0, trace=lambda t, s: got.append(s["info"]))
    return _class_stump(got[0], th.cpu(), C)


class AdaBoost:
    """Multi-class AdaBoost (SAMME) with stumps (daal_adaboost)."""

    def __init__(self, n_rounds=50, learner_depth=1, engine="torch"):
        self.engine = _check_engine(engine)
        self.n_rounds, self.depth = n_rounds, learner_depth
        self.learners, self.alphas = [], []
        self.errors: List[float] = []  # native engine: the weighted error of every learner kept
        self._pack: dict = {}

    def fit(self, X, y, num_classes=None, thresholds=None, trace=None):
        """``thresholds`` / ``trace`` (per round: ``H``, feature, bin, err, alpha) are the
        native engine's; the torch engine raises when given either."""
        K = num_classes or int(y.max()) + 1
        if self.engine == "native":
            return self._fit_native(X, y, int(K), thresholds if thresholds is not None else _bins(X, 256),
                                    trace=trace)
        if thresholds is not None or trace is not None:
            raise ValueError('thresholds / trace need engine="native"')
        n = X.shape[0]
        w = torch.full((n,), 1.0 / n, dtype=torch.float64, device=X.device)
        yl = y.long().to(X.device)
        self.K = K
        for _ in range(self.n_rounds):
            h = DecisionTree("classification", self.depth, n_bins=256).fit(X, yl, w * n, K)
            miss = (h.predict(X) != yl).double()
            err = float((w * miss).sum() / w.sum())
            if err >= 1 - 1.0 / K:
                break
            a = math.log((1 - err) / max(err, 1e-12)) + math.log(K - 1)
            self.learners.append(h)
            self.alphas.append(a)
            w = w * torch.exp(a * miss)
            w = w / w.sum()
            if err < 1e-12:
                break
        return self

    def _fit_native(self, X, y, K: int, th, reduce=None, n_total=None, trace=None):
        """Bin once, then one fused round per stump (``ops.boost.ada_fit``). Deeper learners
        are grown by ``ops.forest.grow`` on the shared bins with the update in torch."""
        n, d = X.shape
        dev = X.device
        B = th.shape[1] + 1
        F.check_shape(B, K)
        self.K = K
        self._pack = {}
        Xb = F.bin_features(X, th)
        if self.depth == 1:
            thc = th.cpu()
            for info in BO.ada_fit(Xb, y.to(dev), d, B, K, self.n_rounds, n_total=n_total, reduce=reduce, trace=trace):
                self.learners.append(_class_stump(info, thc, K))
                self.alphas.append(info[6])
                self.errors.append(info[5])
            return self
        if reduce is not None:
            raise ValueError("fit_distributed supports learner_depth=1 only")
        yl = y.long().to(dev)
        Y = torch.nn.functional.one_hot(yl, K).double()
        w = torch.ones(n, dtype=torch.float64, device=dev)
        one = torch.ones((1, n), dtype=torch.uint8, device=dev)
        proto = DecisionTree("classification", self.depth, n_bins=B, engine="native")
        for _ in range(self.n_rounds):
            packed = F.grow(Xb, d, B, K, F.REAL, one, task=F.GINI, max_depth=self.depth, min_leaf=1.0,
                            stats=Y * w[:, None])
            h = _trees_from_packed(packed, th, proto, [0])[0]
            miss = (F.predict_packed(X, F.pack_trees([h], dev))[0].argmax(1) != yl).double()
            err = float((w * miss).sum() / w.sum())
            if err >= 1 - 1.0 / K:
                break
            a = math.log((1 - err) / max(err, 1e-12)) + math.log(K - 1)
            self.learners.append(h)
            self.alphas.append(a)
            self.errors.append(err)
            w = w * torch.exp(a * miss)
            w = w * (n / w.sum())
            if err < 1e-12:
                break
        return self

    def fit_distributed(self, X, y, comm: Communicator, num_classes=None, thresholds=None):
        """One model over the workers' row shards (native engine, stumps): rank 0's quantiles,
        one histogram all-reduce per round; every worker ends with the same learners."""
        if self.engine != "native":
            raise ValueError('fit_distributed needs engine="native"')
        K, th, n_total = _shards(X, y, comm, num_classes, thresholds, 256)
        return self._fit_native(X, y, K, th, reduce=lambda H: comm.all_reduce(H), n_total=n_total)

    def _decision_packed(self, X):
        """All learners in one pass of the packed-forest kernel: leaf values alpha * e_class."""
        if not self.learners:
            return torch.zeros((X.shape[0], self.K), dtype=torch.float64, device=X.device)
        vals = [a * torch.nn.functional.one_hot(h.value.argmax(1), self.K).double()
                for h, a in zip(self.learners, self.alphas)]
        return _packed_sum(X, self.learners, vals, self.K, self._pack)

    def decision(self, X):
        if self.engine == "native" and X.device.type == "cuda":
            return self._decision_packed(X)
        return self._decision_loop(X)

    def _decision_loop(self, X):
        S = torch.zeros((X.shape[0], self.K), dtype=torch.float64, device=X.device)
        for h, a in zip(self.learners, self.alphas):
            S[torch.arange(X.shape[0], device=X.device), h.predict(X)] += a
        return S

    def predict(self, X):
        return self.decision(X).argmax(1)


def brown_line_search(r, u, s: float, c: float, iters: int, nu: float):
    """The BrownBoost step (alpha, t) for margins ``r``, learner agreement ``u`` (+-1),
    remaining time ``s`` and budget ``c``: t(alpha) keeps the total potential constant, alpha
    zeroes the weighted correlation after the step (nested bisections, every probe read on
    the host)."""

    def pot(z):
        return (1 - torch.erf(z / math.sqrt(c))).sum()

    target = pot(r + s)

    def t_of(a):
        lo, hi = 0.0, s
        if float(pot(r + s - hi + a * u)) <= float(target):
            return hi
        for _ in range(iters):
            mid = 0.5 * (lo + hi)
            if float(pot(r + s - mid + a * u)) < float(target):
                lo = mid
            else:
                hi = mid
        return 0.5 * (lo + hi)

    def corr(a):
        t = t_of(a)
        z = r + s - t + a * u
        return float((torch.exp(-z * z / c) * u).sum()), t

    a_lo, a_hi = 0.0, 1.0
    g_hi, t_hi = corr(a_hi)
    while g_hi > 0 and t_hi < s and a_hi < 1e3:
        a_lo, a_hi = a_hi, a_hi * 2
        g_hi, t_hi = corr(a_hi)
    if g_hi > 0:  # time runs out before the correlation vanishes
        a, t = a_hi, t_hi
    else:
        for _ in range(iters):
            mid = 0.5 * (a_lo + a_hi)
            g, _t = corr(mid)
            if g > 0:
                a_lo = mid
            else:
                a_hi = mid
            if a_hi - a_lo < nu * 1e-3:
                break
        a = 0.5 * (a_lo + a_hi)
        t = t_of(a)
    return a, t


class BrownBoost:
    """Binary BrownBoost (Freund 2001; daal_brownboost): boosting in continuous time with
    a total time budget ``c``. Each round picks the weak learner on weights
    exp(-(r_i + s)^2 / c), then solves for the step (alpha, t): t(alpha) keeps the total
    potential sum_i (1 - erf((r_i + s) / sqrt(c))) constant, alpha zeroes the weighted
    correlation of the learner after the step (both by bisection: robust also when the
    weak learner is nearly perfect). Stops when the remaining time s reaches 0."""

    def __init__(self, c: float = 2.0, max_rounds: int = 100, nu: float = 1e-3, newton_iters: int = 60,
                 engine: str = "torch"):
        self.engine = _check_engine(engine)
        self.c, self.max_rounds, self.nu, self.iters = c, max_rounds, nu, newton_iters
        self.learners, self.alphas = [], []
        self.host_reads: List[int] = []  # native engine: device -> host reads of every round

    def _fit_native(self, X, y, th):
        """Bin once; per round one fused pass (weights exp(-(r + s)^2 / c) from ``r`` and the
        root histogram, scaled to sum n), the split kernels, and ``ops.boost.brown_solve``."""
        n, d = X.shape
        dev = X.device
        B = th.shape[1] + 1
        F.check_shape(B, 2)
        Xb = F.bin_features(X, th)
        thc = th.cpu()
        yi = y.to(dev).int().contiguous()
        ys = (2 * yi - 1).double()
        r = torch.zeros(n, dtype=torch.float64, device=dev)
        rec, mul = BO.new_class_state(dev)
        s = self.c
        for _ in range(self.max_rounds):
            if s <= 1e-9:
                break
            scal = torch.tensor([s, self.c], dtype=torch.float64, device=dev)
            H = BO.class_round(Xb, yi, None, None, None, None, d, B, 2, r=r, scal=scal)
            H = H * (n / H[0, 0].sum())
            bf, bb, _, sp, L, R, T = BO.root_split(H, F.GINI)
            info = BO.class_finish(bf, bb, sp, L, R, T, float(n), rec, mul).tolist()
            if not info[0] or info[5] >= 0.5:  # sum(w u) = S (1 - 2 err) <= 0
                break
            pred = torch.where(Xb[:, int(info[1])] > int(info[2]), int(info[4]), int(info[3]))
            u = (2 * pred - 1).double() * ys
            a, t, reads = BO.brown_solve(r, u, s, self.c, self.iters, self.nu)
            r = r + a * u
            s -= max(t, self.nu)
            self.learners.append(_class_stump(info, thc, 2))
            self.alphas.append(a)
            self.host_reads.append(reads + 1)
        return self

    def fit(self, X, y, thresholds=None):
        if self.engine == "native":
            return self._fit_native(X, y, thresholds if thresholds is not None else _bins(X, 256))
        if thresholds is not None:
            raise ValueError('thresholds need engine="native"')
        yl = y.long().to(X.device)
        ys = (2 * yl - 1).double()  # {-1, +1}
        r = torch.zeros(X.shape[0], dtype=torch.float64, device=X.device)
        s = self.c
        for _ in range(self.max_rounds):
            if s <= 1e-9:
                break
            w = torch.exp(-(r + s) ** 2 / self.c)
            h = DecisionTree("classification", 1, n_bins=256).fit(X, yl, w / w.sum() * X.shape[0], 2)
            u = (2 * h.predict(X) - 1).double() * ys
            if float((w * u).sum()) <= 0:
                break
            a, t = brown_line_search(r, u, s, self.c, self.iters, self.nu)
            r = r + a * u
            s -= max(t, self.nu)
            self.learners.append(h)
            self.alphas.append(a)
        return self

    def decision(self, X):
        out = torch.zeros(X.shape[0], dtype=torch.float64, device=X.device)
        for h, a in zip(self.learners, self.alphas):
            out += a * (2 * h.predict(X) - 1).double()
        return out

    def predict(self, X):
        return (self.decision(X) > 0).long()


class LogitBoost:
    """Multi-class LogitBoost (Friedman, Hastie & Tibshirani 2000; daal_logitboost) with
    regression stumps fit to the Newton working responses."""

    def __init__(self, n_rounds=50, depth=1, zmax=4.0, engine="torch"):
        self.engine = _check_engine(engine)
        self.n_rounds, self.depth, self.zmax = n_rounds, depth, zmax
        self.rounds: List[List[DecisionTree]] = []
        self._pack: dict = {}

    def _fit_native(self, X, y, K: int, th, reduce=None, trace=None):
        """Bin once, then one fused round for all K stumps (``ops.boost.logit_fit``: no host
        read until the end). Deeper learners are grown by ``ops.forest.grow`` on the shared
        bins with the update in torch."""
        n, d = X.shape
        dev = X.device
        B = th.shape[1] + 1
        F.check_shape(B, K)
        self.K = K
        self._pack = {}
        Xb = F.bin_features(X, th)
        if self.depth == 1:
            thc = th.cpu()
            ri, rv, root = BO.logit_fit(Xb, y.to(dev), d, B, K, self.n_rounds, self.zmax, reduce=reduce, trace=trace)
            for t in range(ri.shape[0]):
                fs = []
                for k in range(K):
                    f, b = int(ri[t, k, 0]), int(ri[t, k, 1])
                    fs.append(_stump_tree("regression", B, f >= 0, f, float(thc[f, b]) if f >= 0 else 0.0,
                                          [float(root[t, k]), float(rv[t, k, 0]), float(rv[t, k, 1])]))
                self.rounds.append(fs)
            return self
        if reduce is not None:
            raise ValueError("fit_distributed supports depth=1 only")
        Y = torch.nn.functional.one_hot(y.long().to(dev), K).double()
        Fm = torch.zeros((n, K), dtype=torch.float64, device=dev)
        one = torch.ones((1, n), dtype=torch.uint8, device=dev)
        proto = DecisionTree("regression", self.depth, n_bins=B, engine="native")
        for _ in range(self.n_rounds):
            Pm = torch.softmax(Fm, 1)
            fs = []
            for k in range(K):
                p = Pm[:, k]
                w = (p * (1 - p)).clamp_min(1e-12)
                z = ((Y[:, k] - p) / w).clamp(-self.zmax, self.zmax)
                packed = F.grow(Xb, d, B, 3, F.REAL, one, task=F.MSE, max_depth=self.depth, min_leaf=1.0,
                                stats=torch.stack([w, w * z, w * z * z], 1))
                fs.append(_trees_from_packed(packed, th, proto, [0])[0])
            G = torch.cat([F.predict_packed(X, F.pack_trees([f], dev))[0] for f in fs], 1)
            Fm = Fm + (K - 1) / K * (G - G.mean(1, keepdim=True))
            self.rounds.append(fs)
        return self

    def fit_distributed(self, X, y, comm: Communicator, num_classes=None, thresholds=None):
        """One model over the workers' row shards (native engine, stumps): rank 0's quantiles,
        one histogram all-reduce per round; every worker ends with the same learners."""
        if self.engine != "native":
            raise ValueError('fit_distributed needs engine="native"')
        K, th, _ = _shards(X, y, comm, num_classes, thresholds, 256)
        return self._fit_native(X, y, K, th, reduce=lambda H: comm.all_reduce(H))

    def _decision_packed(self, X):
        """All rounds * K learners in one pass of the packed-forest kernel (learner (t, k)
        carries its value in column k), centred once."""
        K = self.K
        trees = [f for fs in self.rounds for f in fs]
        if not trees:
            return torch.zeros((X.shape[0], K), dtype=torch.float64, device=X.device)
        vals = [f.value * torch.nn.functional.one_hot(torch.tensor(i % K), K).double()[None, :]
                for i, f in enumerate(trees)]
        S = _packed_sum(X, trees, vals, K, self._pack)
        return (K - 1) / K * (S - S.mean(1, keepdim=True))

    def fit(self, X, y, num_classes=None, thresholds=None, trace=None):
        """``thresholds`` / ``trace`` (per round: ``H`` and the K splits) are the native engine's;
        the torch engine raises when given either."""
        K = num_classes or int(y.max()) + 1
        if self.engine == "native":
            return self._fit_native(X, y, int(K), thresholds if thresholds is not None else _bins(X, 256),
                                    trace=trace)
        if thresholds is not None or trace is not None:
            raise ValueError('thresholds / trace need engine="native"')
        self.K = K
        n = X.shape[0]
        Y = torch.nn.functional.one_hot(y.long().to(X.device), K).double()
        F = torch.zeros((n, K), dtype=torch.float64, device=X.device)
        th = _bins(X, 256)
        for _ in range(self.n_rounds):
            Pm = torch.softmax(F, 1)
            fs = []
            for k in range(K):
                p = Pm[:, k]
                w = (p * (1 - p)).clamp_min(1e-12)
                z = ((Y[:, k] - p) / w).clamp(-self.zmax, self.zmax)
                fs.append(DecisionTree("regression", self.depth, n_bins=256).fit(X, z, w, thresholds=th))
            G = torch.stack([f.predict(X) for f in fs], 1)
            G = (K - 1) / K * (G - G.mean(1, keepdim=True))
            F = F + G
            self.rounds.append(fs)
        return self

    def decision(self, X):
        if self.engine == "native" and X.device.type == "cuda":
            return self._decision_packed(X)
        return self._decision_loop(X)

    def _decision_loop(self, X):
        F = torch.zeros((X.shape[0], self.K), dtype=torch.float64, device=X.device)
        for fs in self.rounds:
            G = torch.stack([f.predict(X) for f in fs], 1)
            F += (self.K - 1) / self.K * (G - G.mean(1, keepdim=True))
        return F

    def predict(self, X):
        return self.decision(X).argmax(1)
