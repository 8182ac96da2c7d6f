"""Device test utilities (``csrc/testutil.hip``): a bounded CU hog for rehearsing the
cooperative kernels under CU contention on one GPU, and a one-workgroup kernel that applies
one primitive of ``csrc/wave.h`` to caller-given lanes."""
from __future__ import annotations

import torch

from . import _lib

_lib.register({"harp_test_spin": [_lib.c_int, _lib.c_int, _lib.c_long, _lib.c_void_p, _lib.c_void_p],
               "harp_test_wave": [_lib.c_int, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_int,
                                  _lib.c_void_p]})

# op numbers of wave_test_kernel (csrc/testutil.hip), in its order
WAVE_OPS = ("wave_sum", "wave_sum_d", "wave_sum_i", "wave_max_d", "wave_min_d", "wave_prod_d", "wave_max_f",
            "wave_min_f", "wave_min_u64", "wave_argmax_xor", "wave_argmin_xor", "wave_argmax_dpp", "wave_argmin_dpp",
            "wave_sum_d_dpp", "wave_min_d_dpp", "row_min_d", "row_argmax", "row_argmin", "sub16_sum", "wave_sum_rows",
            "wave_scan_incl", "wave_total", "readlane_d", "block_sum_d", "block_sum_d_pre", "block_max_d_pre",
            "block_argmax", "block_argmin")


def cu_hog(blocks: int, lds_bytes: int, us: int, stream: torch.cuda.Stream) -> torch.Tensor:
    """Launch ``blocks`` 256-thread workgroups on ``stream``, each holding ``lds_bytes`` of
    LDS for ``us`` microseconds; returns the (device) count of finished workgroups."""
    done = torch.zeros(1, dtype=torch.int32, device=stream.device)
    _lib.check(_lib.kernels().harp_test_spin(blocks, lds_bytes, us, done.data_ptr(), stream.cuda_stream), "test_spin")
    return done


def wave_op(op: str, x: torch.Tensor, idx: torch.Tensor):
    """Apply primitive ``op`` (a name of WAVE_OPS) in one workgroup of ``x.numel() / 64`` waves
    (1, 4 or 16): thread t takes (x[t], idx[t]); returns every thread's (fp64, int32) result.
    fp32 primitives work on ``x`` rounded to fp32, wave_min_u64 on the bits of ``x``, readlane_d
    reads the lane ``idx`` of each wave's first thread names."""
    n = x.numel()
    if x.dtype != torch.float64 or idx.dtype != torch.int32 or idx.numel() != n or n not in (64, 256, 1024):
        raise ValueError("wave_op: x fp64 and idx int32 of 64, 256 or 1024 entries")
    if not (x.is_cuda and idx.device == x.device and x.is_contiguous() and idx.is_contiguous()):
        raise ValueError("wave_op: contiguous tensors on one GPU")
    out_d, out_i = torch.empty_like(x), torch.empty_like(idx)
    _lib.check(_lib.kernels().harp_test_wave(WAVE_OPS.index(op), x.data_ptr(), idx.data_ptr(), out_d.data_ptr(),
                                             out_i.data_ptr(), n // 64,
                                             torch.cuda.current_stream(x.device).cuda_stream), "test_wave")
    return out_d, out_i
