"""ctypes mirrors of the route-selection part of include/openr_hip.h and a
thin driver over them (tests/test_gpu_route_kernels.py). Inputs use the data
shapes of tests/route_model.py."""
import ctypes as C

import numpy as np

OK, E_INVALID, E_DEVICE, E_UNSUPPORTED, E_NOMEM, E_STATE = 0, -1, -2, -3, -4, -5
FILL = 0xA5  # output buffers start as this byte: unwritten entries show

u8p, u32p, vp = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.c_void_p


class orh_adv(C.Structure):
    _fields_ = [("name", C.c_uint32), ("meta", C.c_uint32), ("path_pref", C.c_int32),
                ("source_pref", C.c_int32), ("distance", C.c_int32)]


class orh_select_area(C.Structure):
    _fields_ = [("present", C.c_uint32), ("d_dist", vp), ("d_nh", vp), ("d_overloaded", vp),
                ("d_name_node", vp), ("words", C.c_uint32), ("word_off", C.c_uint32)]


class orh_select_out(C.Structure):
    _fields_ = [("d_status", vp), ("d_metric", vp), ("d_best", vp), ("d_mask", vp),
                ("total_words", C.c_uint32)]


class orh_policy(C.Structure):
    _fields_ = [("n_stmts", C.c_uint32), ("stmt_tags", C.c_uint32), ("stmt_prefixes", C.c_uint32),
                ("n_tagsets", C.c_uint32), ("h_tagset_stmts", vp), ("n_pfx", C.c_uint32), ("h_pfx_id", vp),
                ("h_pfx_stmts", vp), ("h_keep", vp), ("total_words", C.c_uint32)]


ADV_DTYPE = np.dtype([("name", "<u4"), ("meta", "<u4"), ("path_pref", "<i4"), ("source_pref", "<i4"),
                      ("distance", "<i4")])
assert C.sizeof(orh_adv) == 20 and ADV_DTYPE.itemsize == 20


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def pack(lists):
    """Advertisement lists -> (adv_ptr u32[n + 1], records, count)."""
    ptr = np.zeros(len(lists) + 1, np.uint32)
    ptr[1:] = np.cumsum([len(a) for a in lists])
    recs = np.zeros(int(ptr[-1]), ADV_DTYPE)
    k = 0
    for advs in lists:
        for name, meta, pp, sp, d in advs:
            recs[k] = (name, meta & 0xFFFFFFFF, _i32(pp), _i32(sp), _i32(d))
            k += 1
    return ptr, recs


def _ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(vp)


class Device:
    """One context; device buffers are freed with it."""

    def __init__(self, lib):
        self.lib = lib
        for name, args in {
            "orh_create": [C.c_int, C.c_uint32, C.POINTER(vp)], "orh_destroy": [vp],
            "orh_device_alloc": [vp, C.c_size_t, C.POINTER(vp)], "orh_device_free": [vp, vp],
            "orh_memcpy_h2d": [vp, vp, vp, C.c_size_t], "orh_memcpy_d2h": [vp, vp, vp, C.c_size_t],
            "orh_sync": [vp], "orh_prefix_create": [vp, C.POINTER(vp)], "orh_prefix_destroy": [vp],
            "orh_prefix_load": [vp, C.c_uint32, vp, vp, vp],
            "orh_prefix_apply_delta": [vp, C.c_uint32, vp, vp, vp, vp],
            "orh_prefix_set_order": [vp, C.c_uint32, vp, C.c_uint32, vp],
            "orh_prefix_info": [vp, u32p, u32p, u32p],
            "orh_route_select": [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.POINTER(orh_select_out)],
            "orh_route_select_range": [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32,
                                       C.POINTER(orh_select_out)],
            "orh_route_diff": [vp, C.c_uint32, C.c_uint32, C.POINTER(orh_select_out),
                               C.POINTER(orh_select_out), vp, vp],
            "orh_route_policy": [vp, C.c_uint32, C.POINTER(orh_select_out), C.POINTER(orh_policy), vp, vp],
            "orh_route_policy_range": [vp, C.c_uint32, C.c_uint32, C.POINTER(orh_select_out),
                                       C.POINTER(orh_policy), vp, vp],
        }.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = args, C.c_int
        lib.orh_last_error.argtypes, lib.orh_last_error.restype = [vp], C.c_char_p
        ctx = vp()
        assert lib.orh_create(0, 0, C.byref(ctx)) == OK
        self.ctx = ctx
        self.bufs = []

    def close(self):
        for d in self.bufs:
            self.lib.orh_device_free(self.ctx, d)
        self.bufs = []
        self.lib.orh_destroy(self.ctx)

    def ok(self, rc):
        assert rc == OK, (rc, self.lib.orh_last_error(self.ctx))

    def alloc(self, nbytes, fill=None):
        d = vp()
        self.ok(self.lib.orh_device_alloc(self.ctx, max(int(nbytes), 4), C.byref(d)))
        self.bufs.append(d)
        if fill is not None and nbytes:
            self.put(d, np.full(int(nbytes), fill, np.uint8))
        return d

    def free(self, *ds):
        for d in ds:
            self.bufs = [b for b in self.bufs if b.value != d.value]
            self.lib.orh_device_free(self.ctx, d)

    def put(self, d, a):
        a = np.ascontiguousarray(a)
        self.ok(self.lib.orh_memcpy_h2d(self.ctx, d, a.ctypes.data_as(vp), a.nbytes))

    def upload(self, a):
        a = np.ascontiguousarray(a)
        d = self.alloc(a.nbytes)
        if a.nbytes:
            self.put(d, a)
        return d

    def get(self, d, dtype, count):
        a = np.zeros(int(count), dtype)
        if a.nbytes:
            self.ok(self.lib.orh_memcpy_d2h(self.ctx, a.ctypes.data_as(vp), d, a.nbytes))
        return a

    # ---- area tables ---------------------------------------------------------
    def areas(self, model_areas):
        """The orh_select_area table of model areas (arrays uploaded)."""
        tab = (orh_select_area * max(len(model_areas), 1))()
        for b, A in enumerate(model_areas):
            tab[b].present, tab[b].words, tab[b].word_off = A["present"], A["words"], A["word_off"]
            if A["name_node"] is not None:
                tab[b].d_name_node = self.upload(np.asarray(A["name_node"], np.uint32))
                tab[b].d_overloaded = self.upload(np.asarray(A["ovl"], np.uint8))
            if A["dist"] is not None:
                tab[b].d_dist = self.upload(np.asarray(A["dist"], np.uint32))
                tab[b].d_nh = self.upload(np.asarray(A["nh"], np.uint32))
        return tab

    def free_areas(self, tab, n):
        for b in range(n):
            for f in ("d_dist", "d_nh", "d_overloaded", "d_name_node"):
                v = getattr(tab[b], f)
                if v:
                    self.free(vp(v))


class Out:
    """A selection output on the device, every byte FILL until written."""

    def __init__(self, dev, n, total_words):
        self.dev, self.n, self.tw = dev, n, total_words
        self.d = [dev.alloc(n, FILL), dev.alloc(4 * n, FILL), dev.alloc(4 * n, FILL),
                  dev.alloc(4 * n * total_words, FILL)]
        self.c = orh_select_out(self.d[0], self.d[1], self.d[2], self.d[3], total_words)

    def read(self):
        g = self.dev.get
        return (g(self.d[0], np.uint8, self.n), g(self.d[1], np.uint32, self.n), g(self.d[2], np.uint32, self.n),
                g(self.d[3], np.uint32, self.n * self.tw).reshape(self.n, self.tw))

    def write(self, status, metric, best, mask):
        for d, a, t in zip(self.d, (status, metric, best, mask), (np.uint8, np.uint32, np.uint32, np.uint32)):
            a = np.ascontiguousarray(np.asarray(a).astype(t))
            if a.nbytes:
                self.dev.put(d, a)

    def free(self):
        self.dev.free(*self.d)


class PrefixSet:
    def __init__(self, dev):
        self.dev = dev
        ps = vp()
        dev.ok(dev.lib.orh_prefix_create(dev.ctx, C.byref(ps)))
        self.ps = ps

    def close(self):
        self.dev.lib.orh_prefix_destroy(self.ps)

    def load(self, prefixes):
        ptr, recs = pack([advs for _, advs in prefixes])
        flags = np.array([f for f, _ in prefixes], np.uint8)
        return self.dev.lib.orh_prefix_load(self.ps, len(prefixes), _ptr(ptr), _ptr(recs), _ptr(flags))

    def delta(self, ids, prefixes):
        ptr, recs = pack([advs for _, advs in prefixes])
        flags = np.array([f for f, _ in prefixes], np.uint8)
        return self.dev.lib.orh_prefix_apply_delta(self.ps, len(ids), _ptr(np.asarray(ids, np.uint32)),
                                                   _ptr(ptr), _ptr(recs), _ptr(flags))

    def set_order(self, name_rank, area_rank):
        nr, ar = np.asarray(name_rank, np.uint32), np.asarray(area_rank, np.uint32)
        return self.dev.lib.orh_prefix_set_order(self.ps, len(nr), _ptr(nr), len(ar), _ptr(ar))

    def info(self):
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self.dev.ok(self.dev.lib.orh_prefix_info(self.ps, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def select(self, me, flags, tab, n_areas, out, lo=None, hi=None):
        if lo is None:
            return self.dev.lib.orh_route_select(self.ps, me, flags, n_areas, C.cast(tab, vp), C.byref(out.c))
        return self.dev.lib.orh_route_select_range(self.ps, me, flags, n_areas, C.cast(tab, vp), lo, hi,
                                                   C.byref(out.c))

    def diff(self, n, prev_n, cur, prev, d_changed, d_count):
        return self.dev.lib.orh_route_diff(self.ps, n, prev_n, C.byref(cur.c), C.byref(prev.c), d_changed, d_count)

    def policy(self, lo, hi, out, pol, total_words, d_out, d_inv, ranged=True):
        """pol: the model's policy dict. The host tables live until the call
        returns (the library copies them)."""
        ts = np.asarray(pol["tagset_stmts"], np.uint32)
        ids = np.asarray(pol["pfx_id"], np.uint32)
        st = np.asarray(pol["pfx_stmts"], np.uint32)
        keep = np.ascontiguousarray(np.asarray(pol["keep"], np.uint32).reshape(-1))
        c = orh_policy(pol["n_stmts"], pol["stmt_tags"], pol["stmt_prefixes"], len(ts), _ptr(ts), len(ids),
                       _ptr(ids), _ptr(st), _ptr(keep), total_words)
        if ranged:
            return self.dev.lib.orh_route_policy_range(self.ps, lo, hi, C.byref(out.c), C.byref(c), d_out, d_inv)
        return self.dev.lib.orh_route_policy(self.ps, hi, C.byref(out.c), C.byref(c), d_out, d_inv)
