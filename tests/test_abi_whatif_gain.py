"""orh_whatif_gain at the C boundary, without a GPU: the header declares it
with its record and options, the record is 80 bytes with the fields where the
tests' numpy mirror has them, the library exports the symbol, and a NULL job is
refused before any device is touched."""
import ctypes
import re

import pytest

from gain_model import FIELDS, REC, U64_FIELDS
from test_abi import HEADER, declared_symbols


@pytest.fixture(scope="module")
def lib():
    from openr_amd import HIP_LIB_PATH
    from openr_amd.build import build_hip_lib
    build_hip_lib()
    return ctypes.CDLL(HIP_LIB_PATH)


class orh_whatif_gain_rec(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64 if f in U64_FIELDS else ctypes.c_uint32) for f in FIELDS]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_gain():
    assert "orh_whatif_gain" in declared_symbols()
    text = _header()
    decl = re.search(r"int orh_whatif_gain\((.*?)\);", text, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert params == ["orh_whatif* job", "uint32_t n_req", "const uint32_t* h_src_idx", "const uint32_t* d_dist",
                      "const uint32_t* d_nh", "const uint32_t* d_info", "const orh_whatif_gain_opts* opts",
                      "orh_whatif_gain_rec* d_out"]
    opts = re.search(r"typedef struct orh_whatif_gain_opts \{(.*?)\} orh_whatif_gain_opts;", text, re.S).group(1)
    assert [" ".join(m.split()) for m in opts.split(";") if m.strip()] == \
        ["const uint32_t* d_weight", "uint32_t* d_node_lost", "uint32_t* d_node_moved", "uint32_t* d_node_nearer"]
    # no comment says any more that the summary is missing
    assert "does not exist yet" not in open(HEADER).read()


def test_record_is_80_bytes_in_the_declared_order():
    body = re.search(r"typedef struct orh_whatif_gain_rec \{(.*?)\} orh_whatif_gain_rec;", _header(), re.S).group(1)
    fields = []
    for stmt in body.split(";"):
        if stmt.strip():
            ctype, names = stmt.split(None, 1)
            fields += [(x.strip(), ctype) for x in names.split(",")]
    assert tuple(f for f, _ in fields) == FIELDS
    assert all(t == ("uint64_t" if f in U64_FIELDS else "uint32_t") for f, t in fields)
    assert ctypes.sizeof(orh_whatif_gain_rec) == 80 == REC.itemsize
    assert ctypes.alignment(orh_whatif_gain_rec) == 8
    for f in FIELDS:
        assert getattr(orh_whatif_gain_rec, f).offset == REC.fields[f][1], f
    # the (max, node) pairs are 8-byte aligned: the kernel maximises one u64 key over each
    assert orh_whatif_gain_rec.max_stretch.offset % 8 == 0 and orh_whatif_gain_rec.max_gain.offset % 8 == 0
    assert orh_whatif_gain_rec.worst_node.offset == orh_whatif_gain_rec.max_stretch.offset + 4
    assert orh_whatif_gain_rec.best_node.offset == orh_whatif_gain_rec.max_gain.offset + 4


def test_library_exports_gain(lib):
    assert hasattr(lib, "orh_whatif_gain")


def test_null_job_is_invalid_without_a_device(lib):
    vp = ctypes.c_void_p
    lib.orh_whatif_gain.argtypes = [vp, ctypes.c_uint32] + [vp] * 6
    lib.orh_whatif_gain.restype = ctypes.c_int
    one = (ctypes.c_uint32 * 2)(0, 0)
    assert lib.orh_whatif_gain(None, 1, one, one, one, None, None, one) == -1
    assert lib.orh_whatif_gain(None, 0, *[None] * 6) == -1
