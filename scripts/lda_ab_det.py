"""A/B of two builds of csrc/lda.hip in the deterministic one-wave modes: the in-tree library
(harp_amd/_native/libharp_kernels.so) against another build (argv[1], e.g. the previous
commit's). Every sampler entry point runs on the same seeded inputs from both libraries and
every output must be bit-identical (a refactor that keeps the samplers' semantics): token
topics, doc-order lists, doc rows, word rows or push payload bytes, topic deltas and the
overflow flag.

  harp_lda_cgs, harp_lda_cgs_ps       variant | 0x100 (chunk order) and | 0x200 (descriptor
                                      order), 8- / 16- / 32-bit doc rows, K = 64, 300, 1000
  harp_lda_cgs_sparse, _span, _span_ps  waves = -1, K = 100, 1100, 4200 (the three word-delta
                                      modes: per-wave rows, one workgroup row, move lists)

Corpus: 3000 docs x 4000 words, about 1e5 tokens."""
import ctypes
import sys

import torch

sys.path.insert(0, ".")
from harp_amd.models.lda import synthetic_corpus  # noqa: E402
from harp_amd.ops import _lib  # noqa: E402
from harp_amd.ops import lda as L  # noqa: E402
from harp_amd.parallel.comm import Communicator  # noqa: E402
from harp_amd.parallel.sparse_ps import SparseRowPS  # noqa: E402

ND, NW = 3000, 4000
ALPHA, BETA, SEED = 0.05, 0.01, 77
DT = {8: torch.uint8, 16: torch.int16, 32: torch.int32}


class State:
    """Seeded inputs for one K: tokens, counts, chunk schedule, parameter-server payloads."""

    def __init__(self, K, dev, max_chunk):
        doc, word = synthetic_corpus(ND, NW, 20, 60, seed=4, device=dev)
        order = torch.argsort(word, stable=True)
        self.K, self.Kp, self.dev = K, L.padded_topics(K), dev
        self.tdoc, self.tword = doc[order].int().contiguous(), word[order].int().contiguous()
        g = torch.Generator(device=dev).manual_seed(1)
        self.tz = torch.randint(0, K, (self.tdoc.numel(),), generator=g, device=dev, dtype=torch.int32)
        self.nwk = torch.zeros((NW, self.Kp), dtype=torch.int32, device=dev)
        nk = torch.zeros(self.Kp, dtype=torch.int32, device=dev)
        L.count(None, self.tword, self.tz, None, self.nwk, nk)
        self.inv = torch.zeros(self.Kp, dtype=torch.float32, device=dev)
        self.inv[:K] = 1.0 / (nk[:K].float() + NW * BETA)
        self.chunks = L.build_chunks(self.tword, max_chunk)
        self.nchunks = self.chunks.numel() - 1
        self.order = L.chunk_order(self.chunks)
        self.di = L.DocIndex.build(self.tdoc, self.tz, ND)
        toks = torch.bincount(self.tword.long().cpu(), minlength=NW)
        self.ps = SparseRowPS(Communicator(None, dev), torch.arange(NW, dtype=torch.int64), toks,
                              lambda x: torch.zeros_like(x), lambda x: x, self.Kp, device=dev)
        self.pbuf = self.ps.pull_payload(self.nwk)
        self.slots = self.ps.row_slots()
        self.qbuf = self.ps.push_payload_buffer()
        self.ndk = {}

    def doc_rows(self, bits):
        if bits not in self.ndk:
            self.ndk[bits] = torch.zeros((ND, self.Kp), dtype=DT[bits], device=self.dev)
            L.count(self.tdoc, None, self.tz, self.ndk[bits])
        return self.ndk[bits]


def run(lib, st, entry, bits=32, variant=0):
    """One sweep of ``entry`` from ``lib`` on copies of the state; the outputs on the host."""
    p = torch.Tensor.data_ptr
    dev, K = st.dev, st.K
    tz, zdoc, nwk, qbuf = st.tz.clone(), st.di.zdoc.clone(), st.nwk.clone(), st.qbuf.clone()
    ndk = st.doc_rows(bits).clone()
    delta = torch.zeros(st.Kp, dtype=torch.int32, device=dev)
    work = torch.zeros(1, dtype=torch.int32, device=dev)
    over = torch.zeros(1, dtype=torch.int32, device=dev)
    poff, pcap, qoff, qcap = st.slots
    fused = (p(st.pbuf), p(poff), p(pcap), p(qbuf), p(qoff), p(qcap), p(over))
    head = (p(st.tword), p(tz), p(st.chunks), st.nchunks)
    tail = (K, ALPHA, BETA, SEED)
    s = torch.cuda.current_stream(dev).cuda_stream
    if entry in ("cgs", "cgs_ps"):
        lpt = L.lpt_desc(st.chunks, st.tword, st.slots if entry == "cgs_ps" else None) if variant & 0x200 else None
        if entry == "cgs":
            rc = lib.harp_lda_cgs(p(st.tdoc), *head, p(ndk), ndk.stride(0), bits, p(nwk), nwk.stride(0), p(st.inv),
                                  p(delta), *tail, variant, _lib.ptr(lpt), s)
        else:
            rc = lib.harp_lda_cgs_ps(p(st.tdoc), *head, p(ndk), ndk.stride(0), bits, p(st.inv), p(delta), *tail,
                                     variant, *fused, _lib.ptr(lpt), s)
    else:
        mid = (p(st.order), p(work), p(st.di.tpos))
        if entry == "sparse":
            rc = lib.harp_lda_cgs_sparse(p(st.tdoc), *head, *mid, p(st.di.doc_off), p(zdoc), p(ndk), ndk.stride(0),
                                         bits, p(nwk), nwk.stride(0), p(st.inv), p(delta), *tail, -1, s)
        elif entry == "sparse_span":
            rc = lib.harp_lda_cgs_sparse_span(p(st.di.span), *head, *mid, p(zdoc), p(nwk), nwk.stride(0), p(st.inv),
                                              p(delta), *tail, -1, s)
        else:
            rc = lib.harp_lda_cgs_sparse_span_ps(p(st.di.span), *head, *mid, p(zdoc), p(st.inv), p(delta), *tail, -1,
                                                 *fused, s)
    torch.cuda.synchronize()
    assert rc == 0, (entry, rc)
    out = {"tz": tz, "zdoc": zdoc, "ndk": ndk, "nwk": nwk, "push": qbuf, "nk_delta": delta, "overflow": over}
    return {k: v.cpu() for k, v in out.items()}


def main():
    dev = torch.device("cuda", 0)
    new = _lib.kernels()
    old = ctypes.CDLL(sys.argv[1])
    _lib._bind(old, _lib._SIGNATURES)
    cases = []
    for K in (64, 300, 1000):
        cases += [(K, e, b, L.SAMPLER_VARIANT | m) for e in ("cgs", "cgs_ps") for b in (8, 16, 32) for m in (0x100, 0x200)]
    for K in (100, 1100, 4200):
        cases += [(K, "sparse", b, 0) for b in (8, 16, 32)] + [(K, "sparse_span", 32, 0), (K, "sparse_span_ps", 32, 0)]
    st, bad = None, 0
    for K, entry, bits, variant in cases:
        if st is None or st.K != K:
            st = State(K, dev, 2048 if K in (64, 300, 1000) else 65536)
        a, b = run(new, st, entry, bits, variant), run(old, st, entry, bits, variant)
        diff = [k for k in a if not torch.equal(a[k], b[k])]
        moved = int((a["tz"] != st.tz.cpu()).sum())
        print(f"K={K} {entry} bits={bits} variant={variant:#x}: moved {moved} of {a['tz'].numel()}, "
              f"overflow {int(a['overflow'])}, differing outputs {diff or 'none'}", flush=True)
        assert moved > 0
        bad += bool(diff)
    assert bad == 0, f"{bad} of {len(cases)} cases differ"
    print(f"all {len(cases)} cases bit-identical")


if __name__ == "__main__":
    main()
