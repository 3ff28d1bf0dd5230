"""orh_whatif_run_metrics at the C boundary, without a GPU: the header
declares it with the orh_whatif_metric record, the library exports it, and a
NULL job is refused before any device is touched."""
import ctypes
import re

import pytest

from test_abi import HEADER, declared_symbols


@pytest.fixture(scope="module")
def lib():
    from openr_amd import HIP_LIB_PATH
    from openr_amd.build import build_hip_lib
    build_hip_lib()
    return ctypes.CDLL(HIP_LIB_PATH)


def test_header_declares_run_metrics():
    assert "orh_whatif_run_metrics" in declared_symbols()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    rec = re.search(r"typedef struct orh_whatif_metric \{(.*?)\} orh_whatif_metric;", text, re.S)
    assert rec, "orh_whatif_metric is not declared"
    assert re.findall(r"uint32_t\s+(\w+);", rec.group(1)) == ["link", "from_node", "metric"]
    decl = re.search(r"int orh_whatif_run_metrics\((.*?)\);", text, re.S).group(1)
    params = [p.split()[-1].lstrip("*") for p in decl.split(",")]
    assert params == ["job", "n_req", "h_src_idx", "h_ignore_ptr", "h_ignore_links", "h_drain_ptr",
                      "h_drain_nodes", "h_metric_ptr", "h_metrics", "d_dist", "d_nh", "d_info"]


def test_library_exports_run_metrics(lib):
    assert hasattr(lib, "orh_whatif_run_metrics")


def test_null_job_is_invalid_without_a_device(lib):
    vp = ctypes.c_void_p
    lib.orh_whatif_run_metrics.argtypes = [vp, ctypes.c_uint32] + [vp] * 10
    lib.orh_whatif_run_metrics.restype = ctypes.c_int
    one = (ctypes.c_uint32 * 2)(0, 0)
    assert lib.orh_whatif_run_metrics(None, 1, one, one, None, None, None, one, None, None, None, None) == -1
    assert lib.orh_whatif_run_metrics(None, 0, None, None, None, None, None, None, None, None, None, None) == -1
