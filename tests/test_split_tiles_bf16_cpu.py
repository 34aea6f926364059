"""Host side of the bf16 split-K tile route: the workspace query (bf16 from 65 rows, the closed form fp16 uses from 33) and the
refusals of the forced variant that return before anything is launched.  No GPU."""
import ctypes

import pytest

from sglang_awq_amd import _lib
from tests.test_host_abi import lib  # noqa: F401  (builds and loads the library)


# min(2 * 256 / wide tiles, 8, 86 / 4, what 32 MiB hold) slices of M x 4096 fp32: 8 / 8 / 4
@pytest.mark.parametrize("M,slices", [(65, 8), (128, 8), (512, 4)])
def test_workspace_query_bf16(lib, M, slices):
    want = 4096 + slices * M * 4096 * 4
    assert lib.awq_gemm_repacked_workspace_bytes(M, 11008, 4096, 128, _lib.DTYPE_BF16) == want
    assert lib.awq_gemm_repacked_workspace_bytes(M, 11008, 4096, 128, _lib.DTYPE_F16) == want
    assert lib.awq_gemm_repacked_workspace_bytes(M, 11008, 4096, 64, _lib.DTYPE_BF16) == 0
    assert lib.awq_gemm_repacked_workspace_bytes(M, 11008, 4096, 128, _lib.DTYPE_F32) == 0


def test_forced_variant_refuses_before_any_launch(lib):
    buf = (ctypes.c_char * 8192)()
    p = ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15)
    call = lambda ws, nbytes, dtype: lib.awq_gemm_repacked_ex(p, 4096, p, None, p, ws, nbytes, 128, 4096, 4096, 128, dtype,
                                                              getattr(_lib, "RP_SPLIT_BF16", 11), None)
    assert call(None, 0, _lib.DTYPE_BF16) == _lib.ERR_BAD_VARIANT       # no workspace
    assert call(p, 4096 + (32 << 20), _lib.DTYPE_F16) == _lib.ERR_BAD_VARIANT
