"""CPU: the batched trace's surface -- the symbols of include/socp_hip.h are declared and exported, socp_amd.capi wraps
them, and capi.trace_kept_rows (the definition of "kept row" that callers and the GPU tests share) agrees with brute force."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("socp_trace_width", "socp_trace_batch_dev", "socp_trace_batch")


def test_symbols_declared_and_exported():
    from socp_amd import capi
    header = open(os.path.join(ROOT, "include", "socp_hip.h")).read()
    L = capi.lib()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(L, name), name
    assert re.search(r"socp_trace_batch_dev\(socp_ctx \*ctx, int B, const double \*d_Z, int stride, int cap, double \*d_rows, int \*d_count\)", header)
    assert re.search(r"socp_trace_batch\(socp_ctx \*ctx, int B, const double \*Z, int stride, int cap, double \*rows, int \*count\)", header)


def test_capi_wrappers():
    from socp_amd import capi
    for name in ("trace_width", "trace_batch_dev", "trace_batch"):
        assert callable(getattr(capi.Context, name)), name
    assert callable(capi.trace_kept_rows)
    L = capi.lib()
    assert len(L.socp_trace_batch_dev.argtypes) == 7 and len(L.socp_trace_batch.argtypes) == 7


@pytest.mark.parametrize("R", [1, 2, 11])
@pytest.mark.parametrize("stride", [1, 4, 10, 25])
def test_kept_rows_against_brute_force(R, stride):
    from socp_amd import capi
    want = [k for k in range(R) if k % stride == 0 or k == R - 1]
    got = capi.trace_kept_rows(R, stride)
    assert list(got) == want
    assert got[0] == 0 and got[-1] == R - 1 and len(set(got)) == len(got)


def test_kept_rows_rejects_nonsense():
    from socp_amd import capi
    for R, stride in ((0, 1), (3, 0), (3, -2)):
        with pytest.raises(ValueError):
            capi.trace_kept_rows(R, stride)
