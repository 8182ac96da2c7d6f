"""Variational LDA E-step (``csrc/lda_vb.hip``), fp64, without a token-by-topic matrix.

Per document (contrib LDAMapper.java:284-327): ``gamma_k = alpha_k + N_d / K``, then passes of
``phi_w = softmax_k(log_beta[., w] + digamma(gamma))``, ``gamma' = alpha + sum_w n_w phi_w``.
With ``tol > 0`` a document stops after its first pass with ``max_k |gamma' - gamma| < tol``
(every document on its own count, at most ``max_passes``); with ``tol == 0`` every document
runs exactly ``max_passes`` passes. One final evaluation at the returned gamma gives
``doc_ll[d] = sum_w n_w logsumexp_k(log_beta[k, w] + digamma(gamma_dk))`` and the word-topic
statistics ``S_t[w, k] = sum_d n_dw phi_dwk``. A document without terms returns
``gamma = alpha``, ``doc_ll = 0`` and one pass.

On a HIP device :func:`estep` launches the native kernels: one wave per document (a
workgroup for a document with more than ``LONG_DOC_TERMS`` terms), gamma in registers, the
``log_beta_t`` rows re-read through L2, so the memory above the inputs is the outputs only.
On CPU tensors it runs :func:`estep_ref`, the same semantics in torch over document batches,
which is also the oracle of the GPU tests.

``S_t`` is accumulated with fp64 global atomics on the GPU: results are reproducible to
rounding, not bitwise (as in ``ops.csr_stats`` and the sparse K-means step).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib

_lib.register({
    "harp_ldavb_max_topics": [],
    "harp_ldavb_long_doc_terms": [],
    # x, out, n, stream
    "harp_ldavb_digamma": [_lib.c_void_p, _lib.c_void_p, _lib.c_long, _lib.c_void_p],
    # rowptr, word, cnt, log_beta_t, alpha, sched, n_docs, n_long, K, max_passes, tol, gamma, passes, doc_ll, S_t,
    # stream
    "harp_ldavb_estep": [_lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p,
                         _lib.c_long, _lib.c_long, _lib.c_int, _lib.c_int, _lib.c_double, _lib.c_void_p,
                         _lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p],
})

MAX_TOPICS = 1024        # LDAVB_MAX_TOPICS in csrc/lda_vb.hip
LONG_DOC_TERMS = 256     # a document with more terms gets a workgroup instead of a wave
GROUP_WIDTHS = (2, 4, 8, 16, 32)  # lanes per term for K <= 32: the next power of two >= K
_REF_CHUNK = 1 << 21     # [terms, K] entries per document batch of the torch reference


def group_width(K: int) -> int:
    """Lanes that work on one term: a sub-wave group for K <= 32, the whole wave above."""
    for g in GROUP_WIDTHS:
        if K <= g:
            return g
    return 64


def _check_topics(K: int) -> None:
    if K < 1 or K > MAX_TOPICS:
        raise ValueError(f"num_topics={K}: the LDA-VB E-step supports 1 <= K <= MAX_TOPICS = {MAX_TOPICS}")


@dataclass
class DocPlan:
    """The document structure of one worker, built once per training run."""
    rowptr: torch.Tensor          # int64 [D + 1]
    word: torch.Tensor            # int32 [nnz], doc-sorted
    doc: torch.Tensor             # int64 [nnz], doc-sorted (non-decreasing)
    sched: torch.Tensor           # int32 [D]: documents longest-first
    n_docs: int
    n_long: int                   # sched[:n_long] have more than LONG_DOC_TERMS terms
    max_word: int                 # -1 without terms
    perm: Optional[torch.Tensor]  # int64 [nnz]: sorted position -> caller's position (None: input was sorted)

    @property
    def long_docs(self) -> torch.Tensor:
        return self.sched[:self.n_long]

    @property
    def nnz(self) -> int:
        return self.word.numel()

    @classmethod
    def build(cls, doc: torch.Tensor, word: torch.Tensor, n_docs: int) -> "DocPlan":
        doc = doc.reshape(-1).long()
        word = word.reshape(-1)
        assert doc.numel() == word.numel()
        if doc.numel():
            if int(doc.min()) < 0 or int(doc.max()) >= n_docs:
                raise ValueError(f"document id outside [0, {n_docs})")
            if int(word.min()) < 0 or int(word.max()) >= 2 ** 31:
                raise ValueError("word id outside [0, 2^31)")
        perm = None
        if doc.numel() > 1 and not bool((doc[1:] >= doc[:-1]).all()):
            perm = torch.argsort(doc, stable=True)
            doc, word = doc[perm], word[perm]
        lengths = torch.bincount(doc, minlength=n_docs)
        if n_docs and int(lengths.max()) >= 2 ** 31 - 1024:  # the kernel's term index is 32-bit and reads ahead
            raise ValueError("a document with 2^31 terms or more")
        rowptr = torch.zeros(n_docs + 1, dtype=torch.long, device=doc.device)
        rowptr[1:] = torch.cumsum(lengths, 0)
        sched = torch.argsort(lengths, descending=True, stable=True).to(torch.int32)
        return cls(rowptr, word.to(torch.int32).contiguous(), doc.contiguous(), sched.contiguous(), int(n_docs),
                   int((lengths > LONG_DOC_TERMS).sum()), int(word.max()) if word.numel() else -1, perm)


def digamma(x: torch.Tensor) -> torch.Tensor:
    """psi(x) for x > 0 in fp64: the device routine of the E-step on a HIP tensor (recurrence up
    to x >= 10, then the asymptotic series through B_14), ``torch.digamma`` on a CPU tensor."""
    assert x.dtype == torch.float64
    if not _lib.use_native(x):
        return torch.digamma(x)
    x = x.contiguous()
    out = torch.empty_like(x)
    _lib.check(_lib.kernels().harp_ldavb_digamma(x.data_ptr(), out.data_ptr(), x.numel(), _lib.stream_ptr(x.device)),
               "ldavb_digamma")
    return out


def estep_ref(plan: DocPlan, cnt: torch.Tensor, log_beta_t: torch.Tensor, alpha: torch.Tensor, max_passes: int,
              tol: float, trace: Optional[list] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Torch implementation of the per-document semantics, in batches of whole documents of at
    most ``_REF_CHUNK`` [terms, K] entries (one document alone may exceed it). A document that
    has met ``tol`` is frozen while the rest of its batch goes on. ``trace`` (a list) receives,
    per pass, the ``max_k |gamma' - gamma|`` of the documents still iterating: the values the
    stopping rule compared with ``tol``."""
    V, K = log_beta_t.shape
    _check_topics(K)
    D, dev, dt = plan.n_docs, log_beta_t.device, log_beta_t.dtype
    if plan.perm is not None:
        cnt = cnt[plan.perm]
    gamma = alpha[None, :].expand(D, K).clone()
    passes = torch.ones(D, dtype=torch.int32, device=dev)
    doc_ll = torch.zeros(D, dtype=dt, device=dev)
    S_t = torch.zeros((V, K), dtype=dt, device=dev)
    per = max(1, _REF_CHUNK // K)
    rp = plan.rowptr.tolist()
    d0 = 0
    while d0 < D:
        d1 = d0 + 1
        while d1 < D and rp[d1 + 1] - rp[d0] <= per:
            d1 += 1
        a, b = rp[d0], rp[d1]
        if b > a:
            n = d1 - d0
            dl = plan.doc[a:b] - d0
            w = plan.word[a:b].long()
            c = cnt[a:b]
            lb = log_beta_t[w]  # [terms of the batch, K]
            Nd = torch.zeros(n, dtype=dt, device=dev).index_add_(0, dl, c)
            g = alpha[None, :] + (Nd / K)[:, None]
            live = Nd.new_ones(n, dtype=torch.bool)
            live &= (plan.rowptr[d0 + 1:d1 + 1] > plan.rowptr[d0:d1])  # an empty document: one pass, gamma = alpha
            npass = torch.ones(n, dtype=torch.int32, device=dev)
            for p in range(1, max_passes + 1):
                phi = torch.softmax(lb + torch.digamma(g)[dl], 1)
                new = alpha[None, :].expand(n, K).clone().index_add_(0, dl, c[:, None] * phi)
                delta = (new - g).abs().amax(1)
                if trace is not None:
                    trace.append(delta[live])
                g = torch.where(live[:, None], new, g)
                npass = torch.where(live, torch.full_like(npass, p), npass)
                if tol > 0:
                    live = live & ~(delta < tol)
                    if not bool(live.any()):
                        break
            lphi = lb + torch.digamma(g)[dl]
            m = lphi.amax(1)
            e = torch.exp(lphi - m[:, None])
            s = e.sum(1)
            doc_ll[d0:d1] = torch.zeros(n, dtype=dt, device=dev).index_add_(0, dl, c * (m + s.log()))
            S_t.index_add_(0, w, e * (c / s)[:, None])
            gamma[d0:d1] = g
            passes[d0:d1] = npass
        d0 = d1
    return gamma, passes, doc_ll, S_t


def estep(plan: DocPlan, cnt: torch.Tensor, log_beta_t: torch.Tensor, alpha: torch.Tensor, max_passes: int,
          tol: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(gamma [D, K], passes [D] int32, doc_ll [D], S_t [V, K])`` for the documents of ``plan``.
    ``cnt`` is in the order of the ``doc`` / ``word`` arrays the plan was built from;
    ``log_beta_t [V, K]`` is word-major and may hold ``-inf`` (a word needs one finite entry).
    The native kernels on HIP tensors, :func:`estep_ref` on CPU tensors. ``S_t`` comes from
    fp64 atomics on the GPU, so its last bits depend on the arrival order."""
    assert log_beta_t.dim() == 2 and log_beta_t.dtype == torch.float64 and cnt.dtype == torch.float64
    V, K = log_beta_t.shape
    _check_topics(K)
    if max_passes < 1 or not tol >= 0:
        raise ValueError(f"max_passes={max_passes}, tol={tol}: need max_passes >= 1 and tol >= 0")
    if cnt.numel() != plan.nnz or alpha.numel() != K:
        raise ValueError("cnt / alpha do not fit the plan / log_beta_t")
    if plan.max_word >= V:
        raise ValueError(f"word id {plan.max_word} outside [0, {V})")
    if not _lib.use_native(log_beta_t):
        return estep_ref(plan, cnt, log_beta_t, alpha, max_passes, tol)
    dev = log_beta_t.device
    assert plan.word.device == dev and cnt.device == dev and alpha.device == dev
    if plan.perm is not None:
        cnt = cnt[plan.perm]
    cnt, lbt, al = cnt.contiguous(), log_beta_t.contiguous(), alpha.to(torch.float64).contiguous()
    D = plan.n_docs
    gamma = torch.empty((D, K), dtype=torch.float64, device=dev)
    passes = torch.empty(D, dtype=torch.int32, device=dev)
    doc_ll = torch.empty(D, dtype=torch.float64, device=dev)
    S_t = torch.zeros((V, K), dtype=torch.float64, device=dev)
    lib = _lib.kernels()
    assert lib.harp_ldavb_max_topics() == MAX_TOPICS and lib.harp_ldavb_long_doc_terms() == LONG_DOC_TERMS
    _lib.check(lib.harp_ldavb_estep(plan.rowptr.data_ptr(), plan.word.data_ptr(), cnt.data_ptr(), lbt.data_ptr(),
                                    al.data_ptr(), plan.sched.data_ptr(), D, plan.n_long, K, int(max_passes),
                                    float(tol), gamma.data_ptr(), passes.data_ptr(), doc_ll.data_ptr(),
                                    S_t.data_ptr(), _lib.stream_ptr(dev)), "ldavb_estep")
    return gamma, passes, doc_ll, S_t
