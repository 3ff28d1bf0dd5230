"""orh_whatif_run_lowers at the C boundary, without a GPU: the header declares
it and the tier it reports, the library exports it, and a NULL job is refused
before any device is touched."""
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


def test_header_declares_run_lowers():
    assert "orh_whatif_run_lowers" in declared_symbols()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+ORH_WHATIF_TIER_LOWERED\s+5u", text)
    decl = re.search(r"int orh_whatif_run_lowers\((.*?)\);", text, re.S).group(1)
    params = [p.split()[-1].lstrip("*") for p in decl.split(",")]
    assert params == ["job", "n_req", "h_src_idx", "h_ignore_ptr", "h_ignore_links", "h_drain_ptr",
                      "h_drain_nodes", "h_metric_ptr", "h_metrics", "h_lower_ptr", "h_lowers", "d_dist", "d_nh",
                      "d_info"]
    assert decl.count("const orh_whatif_metric*") == 2


def test_library_exports_run_lowers(lib):
    assert hasattr(lib, "orh_whatif_run_lowers")


def test_null_job_is_invalid_without_a_device(lib):
    vp = ctypes.c_void_p
    lib.orh_whatif_run_lowers.argtypes = [vp, ctypes.c_uint32] + [vp] * 12
    lib.orh_whatif_run_lowers.restype = ctypes.c_int
    one = (ctypes.c_uint32 * 2)(0, 0)
    assert lib.orh_whatif_run_lowers(None, 1, one, one, None, None, None, None, None, one, None,
                                     None, None, None) == -1
    assert lib.orh_whatif_run_lowers(None, 0, *[None] * 12) == -1
