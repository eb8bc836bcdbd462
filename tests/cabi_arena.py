"""Guarded, deliberately misaligned device buffers for tests of the C ABI (include/pdwt_hip.h) on buffers of a caller.

Two layers:
  * a pure-Python layout planner + a byte checker (`plan`, `fill_pattern`, `check_bytes`), tested without a GPU in
    tests/test_cabi_arena_cpu.py;
  * `Arena`: ONE pdwt_malloc, filled from the host with a position-dependent pattern, payloads uploaded over it; after the driver
    calls `check()` copies the arena back once and compares raw bytes.

A region is a named payload of `elems` elements of `dtype` with a role:
  in       must come back bit-identical         out / inout   written by the driver (values are the test's to compare)
  scratch  any contents afterwards; it KEEPS the fill pattern on upload, so drivers run on d_tmp with arbitrary contents
Every payload starts at a 256-byte aligned address + misalign_elems * itemsize, with `guard_elems` elements of guard in front of and
behind it.  Regions given as a list inside the region list are PACKED: back to back in list order, no gap, guards at the two ends only
(misalign_elems of the first one shifts the group).
"""
import ctypes as C

import numpy as np

ALIGN = 256
# Guard size in elements.  Sized against the widest thing a kernel of pdwt_amd/csrc may stage around a buffer: the 1024-float slot of
# the streaming kernels' trash area (dwt_stream.hpp, kStreamTrashFloats = 256 slots x 1024 floats), which is wider than every tile halo
# (<= 2 * 40 taps * 4 dilation) and than one 16-byte access past the end of an odd-sized band.  A store that misses its buffer by
# up to a whole slot therefore still lands in a guard.  The limit: a store that misses by more than the guard (a whole row of a wide image,
# say) lands in the next payload and goes unreported if that payload is `out`, `inout` or `scratch`; the value comparison of the tests
# is what catches that one.
DEFAULT_GUARD = 1536
ROLES = ("in", "out", "inout", "scratch")


class Region:
    def __init__(self, name, elems, dtype, role, misalign_elems=0, guard_elems=DEFAULT_GUARD):
        assert role in ROLES, role
        self.name, self.elems, self.dtype, self.role = name, int(elems), np.dtype(dtype), role
        self.misalign_elems, self.guard_elems = int(misalign_elems), int(guard_elems)
        self.offset = None  # byte offset of the payload in the arena (set by plan)

    @property
    def nbytes(self):
        return self.elems * self.dtype.itemsize

    def __repr__(self):
        return "Region(%s, %d x %s, %s, +%d, off=%s)" % (self.name, self.elems, self.dtype.name, self.role, self.misalign_elems, self.offset)


def _up(n, a=ALIGN):
    return (n + a - 1) // a * a


def plan(regions):
    """Assign byte offsets.  `regions`: Region objects and/or lists of Regions (a packed group).  Returns (flat list, total bytes)."""
    flat, pos = [], 0
    for item in regions:
        group = list(item) if isinstance(item, (list, tuple)) else [item]
        first, last = group[0], group[-1]
        pos = _up(pos + first.guard_elems * first.dtype.itemsize) + first.misalign_elems * first.dtype.itemsize
        for r in group:
            assert pos % r.dtype.itemsize == 0, (r, pos)  # packed groups share an element type
            r.offset = pos
            pos += r.nbytes
            flat.append(r)
        pos += last.guard_elems * last.dtype.itemsize
    names = [r.name for r in flat]
    assert len(set(names)) == len(names), names
    return flat, _up(pos)


def fill_pattern(nbytes):
    """Position-dependent 32-bit words (an integer hash of the word index): no two guards hold the same bytes, so one guard copied over
    another is a change.  Exponent bits are forced to a finite, normal float32 pattern so that a `scratch` region read as float or
    double holds no NaN / Inf by accident of the hash (kernels must not care, but the references would)."""
    assert nbytes % 4 == 0
    i = np.arange(nbytes // 4, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    w = h.astype(np.uint32)
    w = (w & np.uint32(0x807FFFFF)) | np.uint32(0x3F000000) | ((w >> np.uint32(3)) & np.uint32(0x00800000))  # exponent 126 or 127
    return w.view(np.uint8).copy()


class ArenaDamage(AssertionError):
    pass


def check_bytes(flat, before, after):
    """Compare two uint8 images of the arena.  Every byte outside a payload and every byte of an `in` payload must be unchanged.
    Returns a list of damage reports (empty = clean); each names the region, the side, the first / last damaged byte relative to the
    payload edge and the number of damaged bytes."""
    assert before.shape == after.shape and before.dtype == np.uint8 and after.dtype == np.uint8
    diff = before != after
    reports = []
    order = sorted(flat, key=lambda r: r.offset)
    n = before.size
    for k, r in enumerate(order):
        lo, hi = r.offset, r.offset + r.nbytes
        prev_end = order[k - 1].offset + order[k - 1].nbytes if k else 0
        next_start = order[k + 1].offset if k + 1 < len(order) else n
        # a gap between two payloads is split in the middle: its first half is "behind" the earlier region, the rest "in front of" the later
        front_lo = prev_end + (lo - prev_end + 1) // 2 if k else 0
        back_hi = hi + (next_start - hi + 1) // 2 if k + 1 < len(order) else n
        d = np.flatnonzero(diff[front_lo:lo])
        if d.size:
            reports.append(dict(region=r.name, side="front", first=int(front_lo + d[0] - lo), last=int(front_lo + d[-1] - lo), bytes=int(d.size)))
        d = np.flatnonzero(diff[hi:back_hi])
        if d.size:
            reports.append(dict(region=r.name, side="behind", first=int(d[0]), last=int(d[-1]), bytes=int(d.size)))
        if r.role == "in":
            d = np.flatnonzero(diff[lo:hi])
            if d.size:
                reports.append(dict(region=r.name, side="payload(in)", first=int(d[0]), last=int(d[-1]), bytes=int(d.size)))
    return reports


def format_reports(reports, context=""):
    lines = ["arena damage%s:" % ((" [" + context + "]") if context else "")]
    for r in reports:
        if r["side"] == "front":
            where = "in FRONT of the payload, bytes %d .. %d relative to its first byte" % (r["first"], r["last"])
        elif r["side"] == "behind":
            where = "BEHIND the payload, bytes +%d .. +%d past its last byte" % (r["first"], r["last"])
        else:
            where = "INSIDE the read-only payload, bytes %d .. %d" % (r["first"], r["last"])
        lines.append("  region %-12s %s (%d bytes changed)" % (r["region"], where, r["bytes"]))
    return "\n".join(lines)


def assert_clean(flat, before, after, context=""):
    reports = check_bytes(flat, before, after)
    if reports:
        raise ArenaDamage(format_reports(reports, context))


class Arena:
    """One device allocation holding every buffer of a driver call.  payloads: {name: numpy array} for every non-scratch region (an
    `out` region may be left out: it then keeps the pattern, which a forward must overwrite completely)."""

    def __init__(self, L, regions, payloads=None):
        self.L = L
        self.flat, self.nbytes = plan(regions)
        self.by_name = {r.name: r for r in self.flat}
        self.host = fill_pattern(self.nbytes)
        for name, arr in (payloads or {}).items():
            self._put(name, arr)
        self.base = L.pdwt_malloc(self.nbytes)
        assert self.base, "pdwt_malloc(%d)" % self.nbytes
        assert self.base % ALIGN == 0, hex(self.base)
        assert L.pdwt_memcpy_h2d(self.base, self.host.ctypes.data, self.nbytes) == 0

    def _put(self, name, arr):
        r = self.by_name[name]
        a = np.ascontiguousarray(arr, dtype=r.dtype).reshape(-1)
        assert a.size <= r.elems, (name, a.size, r.elems)
        self.host[r.offset:r.offset + a.nbytes] = a.view(np.uint8)

    def upload(self, name, arr):
        """overwrite (the start of) a payload on the device and in the `before` image"""
        self._put(name, arr)
        r = self.by_name[name]
        assert self.L.pdwt_memcpy_h2d(self.base + r.offset, self.host[r.offset:].ctypes.data, r.nbytes) == 0

    def ptr(self, name):
        return self.base + self.by_name[name].offset

    def band_table(self, names, ct):
        P = C.POINTER(ct)
        return (P * len(names))(*[C.cast(self.ptr(n), P) for n in names])

    def download(self):
        out = np.empty(self.nbytes, dtype=np.uint8)
        assert self.L.pdwt_memcpy_d2h(out.ctypes.data, self.base, self.nbytes) == 0
        return out

    def check(self, context=""):
        """one copy back; guards and `in` payloads byte for byte.  Returns the downloaded image (use `get` on it).  The downloaded image
        becomes the new `before` (also when damage is reported), so a following call on the same arena is checked against what this
        one left.  The role of a region may be changed between calls (by_name[name].role)."""
        after = self.download()
        before, self.host = self.host, after
        assert_clean(self.flat, before, after, context)
        return after

    def get(self, image, name, elems=None, shape=None):
        r = self.by_name[name]
        n = r.elems if elems is None else int(elems)
        a = image[r.offset:r.offset + n * r.dtype.itemsize].view(r.dtype).copy()
        return a.reshape(shape) if shape is not None else a

    def free(self):
        if self.base:
            self.L.pdwt_sync()
            self.L.pdwt_free(self.base)
            self.base = None
