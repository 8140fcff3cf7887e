"""The shared scans and the radix sort of pch_prims.hip behind their self-test entries, against the numpy statements
of tests/prims_cases.py: every result is an integer and every comparison is equality.  Outputs are slices of larger
buffers with 64 guard words on each side, which must read as before."""
import ctypes

import numpy as np
import pytest
import torch

import prims_cases as pc
from pointcloudhookup_amd import _lib, ops

pytestmark = pytest.mark.gpu

FILL32 = pc.GUARD_WORD - 2 ** 32                               # the guard word as int32 / twice as int64
FILL64 = (pc.GUARD_WORD << 32 | pc.GUARD_WORD) - 2 ** 64


class Guarded:
    """n elements of int32 / int64 at a 16-byte aligned offset of a buffer that is guard words everywhere else"""
    def __init__(self, n, dtype, cuda):
        per = 2 if dtype == torch.int64 else 1                 # 32-bit words per element
        self.n, self.g = n, pc.GUARD // per
        self.fill = FILL64 if per == 2 else FILL32
        pad = -(-n * per // 4) * 4 // per                      # the guard behind starts at a 16-byte aligned offset too
        self.buf = torch.full((self.g + pad + self.g,), self.fill, dtype=dtype, device=cuda)
        self.view = self.buf[self.g:self.g + n]
        assert self.view.data_ptr() % 16 == 0 or n == 0

    def host(self, np_dtype):
        return self.view.cpu().numpy().view(np_dtype)

    def check_guards(self, what=""):
        h = self.buf.cpu().numpy()
        assert np.all(h[:self.g] == self.fill), f"{what}: guard words in front of the output were written"
        assert np.all(h[self.g + self.n:] == self.fill), f"{what}: guard words behind the output were written"

    def check_untouched(self, what=""):
        assert bool((self.buf == self.fill).all()), f"{what}: a refused call wrote to the buffer"


def _dev_u32(v, cuda):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint32).view(np.int32)).to(cuda)


def _dev_u64(v, cuda):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint64).view(np.int64)).to(cuda)


def _run_scan(cuda, v, form, in_place=False, with_total=True, calls=1):
    """-> [(out uint32 [n], total or None)] of `calls` identical calls, guards checked"""
    n = len(v)
    out = Guarded(n, torch.int32, cuda)
    total = Guarded(1, torch.int32, cuda)                       # starts as the guard word, not as zero
    if in_place:
        out.view.copy_(_dev_u32(v, cuda))
        inp = out.view
    else:
        inp = _dev_u32(v, cuda)
    got = []
    for _ in range(calls):
        ops.selftest_scan_u32(inp, out.view, form, total.view if with_total else None)
        got.append((out.host(np.uint32), int(total.host(np.uint32)[0]) if with_total else None))
    out.check_guards("out")
    if with_total:
        total.check_guards("out_total")
    else:
        total.check_untouched("out_total")
    if not in_place:
        np.testing.assert_array_equal(inp.cpu().numpy().view(np.uint32), v, err_msg="the input was written")
    return got


def _check_scan(cuda, form, n, kind, **kw):
    popc = form in (1, 3)
    v = pc.scan_values(kind, n, popc)
    want, want_total = pc.scan_reference(pc.scanned(v, popc))
    for out, total in _run_scan(cuda, v, form, **kw):
        np.testing.assert_array_equal(out, want, err_msg=f"form {form}, n {n}, {kind}")
        if total is not None:
            assert total == want_total, (form, n, kind)


# ------------------------------------------------------------------ three-launch scan
@pytest.mark.parametrize("n", pc.SCAN3_SIZES)
def test_scan_three_launch(cuda, n):
    for kind in pc.SCAN_VALUES:
        _check_scan(cuda, 0, n, kind)
    if n > 0:
        _check_scan(cuda, 0, n, "wrap")                         # total in [2^31, 2^32)


@pytest.mark.parametrize("n", pc.SCAN3_SIZES)
def test_scan_three_launch_in_place(cuda, n):
    for kind in ("ones", "small", "spike"):
        _check_scan(cuda, 0, n, kind, in_place=True)


@pytest.mark.parametrize("n", pc.SCAN3_SIZES)
def test_scan_three_launch_popcount(cuda, n):
    for kind in pc.POPC_VALUES:
        _check_scan(cuda, 1, n, kind)


@pytest.mark.parametrize("form", [0, 1, 2, 3, 4])
def test_scan_without_total(cuda, form):
    for n in (0, 9, 3 * pc.TILE + 5):
        _check_scan(cuda, form, n, "small", with_total=False)


# ------------------------------------------------------------------ one-launch (look-back) scan
@pytest.mark.parametrize("form", [2, 3])
@pytest.mark.parametrize("n", pc.SCAN1_SIZES)
def test_scan_one_launch(cuda, form, n):
    """the same call twice on the same buffers: the entry zeroes status words, ticket and total each time"""
    for kind in (pc.POPC_VALUES if form == 3 else pc.SCAN_VALUES):
        _check_scan(cuda, form, n, kind, calls=2)


@pytest.mark.parametrize("n", pc.SCAN1_SIZES)
def test_scan_one_launch_in_place(cuda, n):
    for kind in ("ones", "small", "spike"):
        _check_scan(cuda, 2, n, kind, in_place=True)


# ------------------------------------------------------------------ the tile-sum scan alone
@pytest.mark.parametrize("n", pc.TILE_SUM_SIZES)
def test_scan_tile_sums(cuda, n):
    for kind in pc.SCAN_VALUES:
        _check_scan(cuda, 4, n, kind)
    _check_scan(cuda, 4, n, "small", in_place=True)


# ------------------------------------------------------------------ radix sort
def _run_sort(cuda, keys, vals, nbits):
    n = len(keys)
    ok, ov = Guarded(n, torch.int64, cuda), Guarded(n, torch.int32, cuda)
    dk, dv = _dev_u64(keys, cuda), _dev_u32(vals, cuda)
    ops.selftest_radix_sort_pairs(dk, dv, nbits, ok.view, ov.view)
    got = ok.host(np.uint64), ov.host(np.uint32)
    ok.check_guards("out_keys")
    ov.check_guards("out_vals")
    np.testing.assert_array_equal(dk.cpu().numpy().view(np.uint64), keys, err_msg="the input keys were written")
    np.testing.assert_array_equal(dv.cpu().numpy().view(np.uint32), vals, err_msg="the input values were written")
    return got


@pytest.mark.parametrize("kind,n,nbits", pc.sort_cases())
def test_radix_sort_pairs(cuda, kind, n, nbits):
    keys, vals = pc.sort_keys(kind, n, nbits)
    want_k, want_v = pc.sort_reference(keys, vals, nbits)
    got_k, got_v = _run_sort(cuda, keys, vals, nbits)
    np.testing.assert_array_equal(got_k, want_k)
    np.testing.assert_array_equal(got_v, want_v)
    if nbits == 0 or kind in ("equal", "high_only", "crop_fill"):          # nothing to order by: the input order
        np.testing.assert_array_equal(got_k, keys)
        np.testing.assert_array_equal(got_v, vals)


# ------------------------------------------------------------------ refusals
def test_refusals_write_nothing(cuda):
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    ARG, WS = -1, -2

    def refused(rc, code, text=None):
        assert rc == code, (rc, L.pch_last_error())
        if text:
            assert text in L.pch_last_error().decode()

    n = 3 * pc.TILE + 5
    src = Guarded(n, torch.int32, cuda)                                     # also the aliased output of form 1 / 3
    out, total = Guarded(n, torch.int32, cuda), Guarded(1, torch.int32, cuda)
    host = np.zeros(n + 8, dtype=np.uint32)
    i, o, t = src.view.data_ptr(), out.view.data_ptr(), total.view.data_ptr()
    for form in range(5):
        need = L.pch_selftest_scan_u32_ws_bytes(n, form)
        assert need > 0
        ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=cuda)
        w = ws.data_ptr()
        refused(L.pch_selftest_scan_u32(None, o, n, form, t, w, need, stream), ARG, "null")
        refused(L.pch_selftest_scan_u32(i, None, n, form, t, w, need, stream), ARG, "null")
        refused(L.pch_selftest_scan_u32(i, o, n, form, t, None, need, stream), ARG, "null")
        refused(L.pch_selftest_scan_u32(i, o, -1, form, t, w, need, stream), ARG, "size")
        refused(L.pch_selftest_scan_u32(i, o, 2 ** 31, form, t, w, need, stream), ARG, "size")
        refused(L.pch_selftest_scan_u32(i, o, n, form, t, w, need - 1, stream), WS, "workspace too small")
        refused(L.pch_selftest_scan_u32(host.ctypes.data_as(ctypes.c_void_p), o, n, form, t, w, need, stream), ARG,
                "device pointer")
        refused(L.pch_selftest_scan_u32(i + 4, o, n - 1, form, t, w, need, stream), ARG, "aligned")
        refused(L.pch_selftest_scan_u32(i, o + 4, n - 1, form, t, w, need, stream), ARG, "aligned")
        refused(L.pch_selftest_scan_u32(i, i + 16, n - 4, form, t, w, need, stream), ARG, "overlap")
        if form in (1, 3):
            refused(L.pch_selftest_scan_u32(i, i, n, form, t, w, need, stream), ARG, "in place")
        assert bool((ws == 0x5A).all()), "a refused call wrote to the workspace"
    need = L.pch_selftest_scan_u32_ws_bytes(n, 0)
    for form in (-1, 5):
        assert L.pch_selftest_scan_u32_ws_bytes(n, form) == 0
        refused(L.pch_selftest_scan_u32(i, o, n, form, t, ws.data_ptr(), need, stream), ARG, "form")
    assert L.pch_selftest_scan_u32_ws_bytes(-1, 0) == 0 and L.pch_selftest_radix_sort_ws_bytes(-1) == 0

    keys, vals = Guarded(n, torch.int64, cuda), Guarded(n, torch.int32, cuda)
    ok, ov = Guarded(n, torch.int64, cuda), Guarded(n, torch.int32, cuda)
    need = L.pch_selftest_radix_sort_ws_bytes(n)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=cuda)
    k, v, pk, pv, w = (x.data_ptr() for x in (keys.view, vals.view, ok.view, ov.view, ws))
    hostk = np.zeros(n, dtype=np.uint64)
    good = [k, v, n, 17, pk, pv, w, need, stream]
    for at in (0, 1, 4, 5, 6):
        refused(L.pch_selftest_radix_sort_pairs(*(good[:at] + [None] + good[at + 1:])), ARG, "null")
    for at, bad, code, text in ((2, -1, ARG, "size"), (2, 2 ** 31, ARG, "size"), (3, -1, ARG, "nbits"),
                                (3, 65, ARG, "nbits"), (7, need - 1, WS, "workspace too small"),
                                (0, hostk.ctypes.data_as(ctypes.c_void_p), ARG, "device pointer"),
                                (0, k + 4, ARG, "aligned"), (4, pk + 4, ARG, "aligned")):
        refused(L.pch_selftest_radix_sort_pairs(*(good[:at] + [bad] + good[at + 1:])), code, text)
    assert bool((ws == 0x5A).all()), "a refused call wrote to the workspace"

    torch.cuda.synchronize()
    for name, b in (("in", src), ("out", out), ("out_total", total), ("keys", keys), ("vals", vals),
                    ("out_keys", ok), ("out_vals", ov)):
        b.check_untouched(name)
    assert not host.any() and not hostk.any()
