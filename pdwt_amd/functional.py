"""Differentiable boundary-mode DWT for torch device tensors: a stateless layer over the C-ABI drivers of include/pdwt_hip.h
("Batched 2-D / 1-D DWT with boundary modes", "Batched 3-D DWT with boundary modes" and the "Adjoints ..." sections).

    bands = dwt2(x, "db2", levels=2, mode="symmetric")   # x: (..., Nr, Nc) -> [A_L, H1, V1, D1, ..., H_L, V_L, D_L], each (..., nr_l, nc_l)
    x     = idwt2(bands, (Nr, Nc), "db2")
    bands = dwt1(x, "db4", levels=3, mode="periodic")    # x: (..., n) along the last axis -> [A_L, D_1, ..., D_L]
    x     = idwt1(bands, n, "db4")
    bands = dwt3(x, "db2", levels=2, mode="symmetric")   # x: (..., Nz, Nr, Nc) -> [A_L, 7 details of level L, ..., 7 details of level 1]
    x     = idwt3(bands, (Nz, Nr, Nc), "db2")            # (COARSEST level first, unlike dwt2: the table of BoundaryWavelets3D)

The six transforms are ``torch.autograd.Function``s (once differentiable): they accept ``requires_grad`` inputs and take part in a graph;
their backward is the matching adjoint operator, which is also exposed bare: ``dwt2_adjoint``, ``idwt2_adjoint``, ``dwt1_adjoint``,
``idwt1_adjoint``, ``dwt3_adjoint``, ``idwt3_adjoint``.  With a signal extension the adjoint of the forward transform is not the inverse.

Tensors must be contiguous float32 / float64 tensors on the GPU (``TypeError`` otherwise); outputs and scratch are torch allocations.
Nothing is clamped: ``levels < 1``, a level whose axis is shorter than ``hlen - 1``, an unknown mode or wavelet, or a band list of the
wrong length or shapes raise ``ValueError`` before anything is launched.  The library runs on its own stream: every call waits for torch's
current stream before it starts (the producer) and for the library stream before it returns (the consumer).  torch is imported on first use.
"""
import ctypes as C

from . import _native as N
from .wavelets import _sync_producer

MODES = ("zero", "constant", "symmetric", "reflect", "periodic")
MAX_LEVELS = 32
MAX_BATCH = 65535
MAX_LEVELS_3D = 13
KEYS_3D = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")  # a level's details in table order (first letter: the z axis, a = low pass)

__all__ = ["dwt2", "idwt2", "dwt1", "idwt1", "dwt3", "idwt3", "dwt2_adjoint", "idwt2_adjoint", "dwt1_adjoint", "idwt1_adjoint", "dwt3_adjoint",
           "idwt3_adjoint", "MODES"]

_banks = {}
_fn = None


def _torch():
    import torch
    return torch


# ---- argument checks (no launch) ------------------------------------------------------------------------------------------------
def _sfx(t):
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        raise TypeError("a torch tensor is required, not %s" % type(t).__name__)
    if not t.is_cuda:
        raise TypeError("the tensor must live on the GPU (pdwt_amd has no CPU path)")
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError("the tensor must be float32 or float64, not %s" % t.dtype)
    if not t.is_contiguous():
        raise TypeError("the tensor must be contiguous")
    return "f32" if t.dtype == torch.float32 else "f64"


def _bank(wname, sfx):
    key = (str(wname).lower(), sfx)
    if key not in _banks:
        f = (N.Filters32 if sfx == "f32" else N.Filters64)()
        hlen = getattr(N.hip(), "pdwt_compute_filters_separable_" + sfx)(key[0].encode(), 0, C.byref(f))
        if hlen < 2:
            raise ValueError("unknown wavelet %r" % (wname,))
        f.hlen = hlen
        _banks[key] = f
    return _banks[key]


def _mode(mode):
    if mode not in MODES:
        raise ValueError("unknown mode %r (one of %s)" % (mode, ", ".join(MODES)))
    return MODES.index(mode)


def _levels(levels, most=MAX_LEVELS):
    if int(levels) != levels or not 1 <= int(levels) <= most:
        raise ValueError("levels must be 1 .. %d, not %r" % (most, levels))
    return int(levels)


def _axis_lengths(n, hlen, levels, what):
    """[n_0, ..., n_levels]; every level's input at least hlen - 1 long"""
    out = [int(n)]
    for l in range(levels):
        if out[-1] < max(hlen - 1, 1):
            raise ValueError("level %d: the %s axis has %d samples, fewer than hlen - 1 = %d (levels are not clamped)" % (l + 1, what, out[-1], hlen - 1))
        out.append((out[-1] + hlen - 1) // 2)
    return out


def _count(lead, limit, what):
    b = 1
    for v in lead:
        b *= int(v)
    if not 1 <= b <= limit:
        raise ValueError("%d %s: 1 .. %d are supported" % (b, what, limit))
    return b


def _band_list(bands, per_level, most=MAX_LEVELS):
    torch = _torch()
    if not isinstance(bands, (list, tuple)) or len(bands) < per_level + 1 or (len(bands) - 1) % per_level:
        raise ValueError("a band list of %d * levels + 1 tensors is required" % per_level)
    sfx = _sfx(bands[0])
    for b in bands[1:]:
        if _sfx(b) != sfx or b.device != bands[0].device:
            raise ValueError("the bands must share dtype and device")
    return list(bands), sfx, _levels((len(bands) - 1) // per_level, most)


def _check_shapes(bands, lead, shapes):
    for k, (b, s) in enumerate(zip(bands, shapes)):
        if tuple(b.shape) != tuple(lead) + tuple(s):
            raise ValueError("band %d has shape %s, expected %s" % (k, tuple(b.shape), tuple(lead) + tuple(s)))


def _table(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _run(name, sfx, like, tmp_elems, call):
    """allocate the scratch, order the library stream after torch's and torch after the library's"""
    torch = _torch()
    L = N.hip()
    if like.device.index is not None and like.device.index != L.pdwt_get_device():
        raise ValueError("the tensors live on device %d, the library runs on device %d (pdwt_set_device)" % (like.device.index, L.pdwt_get_device()))
    if tmp_elems < 0:
        raise ValueError("%s: sizes the drivers refuse" % name)
    tmp = torch.empty(int(tmp_elems), dtype=like.dtype, device=like.device) if tmp_elems else None
    _sync_producer()
    rc = call(getattr(L, "pdwt_%s_%s" % (name, sfx)), C.c_void_p(tmp.data_ptr()) if tmp is not None else None)
    if rc < 0:
        raise RuntimeError("pdwt_%s_%s failed (%d): %s" % (name, sfx, rc, (L.pdwt_last_error_string() or b"").decode()))
    if L.pdwt_sync() != 0:
        raise RuntimeError("pdwt_sync failed: %s" % (L.pdwt_last_error_string() or b"").decode())
    return rc


# ---- the eight operators on plain tensors (no autograd) -------------------------------------------------------------------------------
def _geom2(shape2, hlen, levels):
    rs = _axis_lengths(shape2[0], hlen, levels, "row")
    cs = _axis_lengths(shape2[1], hlen, levels, "column")
    return [(rs[levels], cs[levels])] + [(rs[l], cs[l]) for l in range(1, levels + 1) for _ in range(3)]


def _shape2(shape):
    if len(shape) != 2 or int(shape[0]) < 1 or int(shape[1]) < 1:
        raise ValueError("shape must be (Nr, Nc), not %r" % (tuple(shape),))
    return int(shape[0]), int(shape[1])


def _dwt2(x, wname, levels, mode, adjoint_of_inverse=False):
    sfx = _sfx(x)
    if x.dim() < 2:
        raise ValueError("a tensor of shape (..., Nr, Nc) is required")
    levels, f = _levels(levels), _bank(wname, sfx)
    m = 0 if adjoint_of_inverse else _mode(mode)
    lead, (Nr, Nc) = tuple(x.shape[:-2]), _shape2(x.shape[-2:])
    shapes = _geom2((Nr, Nc), f.hlen, levels)
    B = _count(lead, MAX_BATCH, "images")
    L = N.hip()
    bands = [x.new_empty(lead + s) for s in shapes]
    tab = _table(bands)
    tmp = L.pdwt_ext2db_tmp_elems(B, Nr, Nc, f.hlen, levels, x.element_size())
    if adjoint_of_inverse:
        _run("ext2db_inverse_adjoint", sfx, x, tmp, lambda fn, t: fn(C.c_void_p(x.data_ptr()), tab, B, Nr, Nc, levels, C.byref(f), t))
    else:
        _run("ext2db_forward", sfx, x, tmp, lambda fn, t: fn(C.c_void_p(x.data_ptr()), tab, B, Nr, Nc, levels, m, C.byref(f), t))
    return bands


def _idwt2(bands, shape, wname, mode=None):
    """mode None: the inverse; a mode: the adjoint of the forward transform"""
    bands, sfx, levels = _band_list(bands, 3)
    f = _bank(wname, sfx)
    m = None if mode is None else _mode(mode)
    Nr, Nc = _shape2(shape)
    shapes = _geom2((Nr, Nc), f.hlen, levels)
    if bands[0].dim() < 2:
        raise ValueError("bands of shape (..., nr, nc) are required")
    lead = tuple(bands[0].shape[:-2])
    _check_shapes(bands, lead, shapes)
    B = _count(lead, MAX_BATCH, "images")
    L = N.hip()
    out = bands[0].new_empty(lead + (Nr, Nc))
    tab = _table(bands)
    es = bands[0].element_size()
    if m is None:
        _run("ext2db_inverse", sfx, out, L.pdwt_ext2db_tmp_elems(B, Nr, Nc, f.hlen, levels, es),
             lambda fn, t: fn(C.c_void_p(out.data_ptr()), tab, B, Nr, Nc, levels, C.byref(f), t))
    else:
        _run("ext2db_forward_adjoint", sfx, out, L.pdwt_ext2db_adjoint_tmp_elems(B, Nr, Nc, f.hlen, levels, es),
             lambda fn, t: fn(C.c_void_p(out.data_ptr()), tab, B, Nr, Nc, levels, m, C.byref(f), t))
    return out


def _rows(lead, n):
    rows = _count(lead, (1 << 31) - 1, "rows")
    if rows * n >= 1 << 31:
        raise ValueError("%d rows of %d samples: fewer than 2^31 elements are supported" % (rows, n))
    return rows


def _dwt1(x, wname, levels, mode, adjoint_of_inverse=False):
    sfx = _sfx(x)
    if x.dim() < 1:
        raise ValueError("a tensor of shape (..., n) is required")
    levels, f = _levels(levels), _bank(wname, sfx)
    m = 0 if adjoint_of_inverse else _mode(mode)
    lead, n = tuple(x.shape[:-1]), int(x.shape[-1])
    ns = _axis_lengths(n, f.hlen, levels, "last")
    rows = _rows(lead, n)
    L = N.hip()
    bands = [x.new_empty(lead + (k,)) for k in [ns[levels]] + ns[1:]]
    tab = _table(bands)
    tmp = L.pdwt_ext1d_tmp_elems(rows, n, f.hlen, levels, x.element_size())
    if adjoint_of_inverse:
        _run("ext1d_inverse_adjoint", sfx, x, tmp, lambda fn, t: fn(C.c_void_p(x.data_ptr()), tab, rows, n, levels, C.byref(f), t))
    else:
        _run("ext1d_forward", sfx, x, tmp, lambda fn, t: fn(C.c_void_p(x.data_ptr()), tab, rows, n, levels, m, C.byref(f), t))
    return bands


def _idwt1(bands, n, wname, mode=None):
    bands, sfx, levels = _band_list(bands, 1)
    f = _bank(wname, sfx)
    m = None if mode is None else _mode(mode)
    if int(n) != n or int(n) < 1:
        raise ValueError("n must be a positive integer, not %r" % (n,))
    n = int(n)
    ns = _axis_lengths(n, f.hlen, levels, "last")
    if bands[0].dim() < 1:
        raise ValueError("bands of shape (..., N) are required")
    lead = tuple(bands[0].shape[:-1])
    _check_shapes(bands, lead, [(k,) for k in [ns[levels]] + ns[1:]])
    rows = _rows(lead, n)
    L = N.hip()
    out = bands[0].new_empty(lead + (n,))
    tab = _table(bands)
    es = bands[0].element_size()
    if m is None:
        _run("ext1d_inverse", sfx, out, L.pdwt_ext1d_tmp_elems(rows, n, f.hlen, levels, es),
             lambda fn, t: fn(C.c_void_p(out.data_ptr()), tab, rows, n, levels, C.byref(f), t))
    else:
        _run("ext1d_forward_adjoint", sfx, out, L.pdwt_ext1d_adjoint_tmp_elems(rows, n, f.hlen, levels, es),
             lambda fn, t: fn(C.c_void_p(out.data_ptr()), tab, rows, n, levels, m, C.byref(f), t))
    return out


# ---- 3-D: a stack of volumes per driver call (the leading axes are the stack; the drivers loop the levels) -------------------------------
def _shape3(shape):
    if len(shape) != 3 or any(int(v) != v or int(v) < 1 for v in shape):
        raise ValueError("shape must be (Nz, Nr, Nc), not %r" % (tuple(shape),))
    return tuple(int(v) for v in shape)


def _geom3(shape3, hlen, levels):
    """[(nz_l, nr_l, nc_l) for l = 0 .. levels]: every level is one the level entries and their adjoints take"""
    axes = [_axis_lengths(n, hlen, levels, what) for n, what in zip(shape3, ("z", "row", "column"))]
    shapes = [tuple(a[l] for a in axes) for l in range(levels + 1)]
    L = N.hip()
    for l in range(levels):
        if L.pdwt_ext3d_adjoint_level_tmp_elems(shapes[l][0], shapes[l][1], shapes[l][2], hlen) < 0:
            raise ValueError("level %d: a %d x %d x %d volume is a size the level drivers refuse" % ((l + 1,) + shapes[l]))
    return shapes


def _table_shapes3(shapes, levels):
    return [shapes[levels]] + [shapes[l] for l in range(levels, 0, -1) for _ in range(7)]


def _dwt3(x, wname, levels, mode, adjoint_of_inverse=False):
    sfx = _sfx(x)
    if x.dim() < 3:
        raise ValueError("a tensor of shape (..., Nz, Nr, Nc) is required")
    levels, f = _levels(levels, MAX_LEVELS_3D), _bank(wname, sfx)
    m = 0 if adjoint_of_inverse else _mode(mode)
    lead, (Nz, Nr, Nc) = tuple(x.shape[:-3]), _shape3(x.shape[-3:])
    shapes = _geom3((Nz, Nr, Nc), f.hlen, levels)
    V = _count(lead, (1 << 31) - 1, "volumes")
    L = N.hip()
    bands = [x.new_empty(lead + s) for s in _table_shapes3(shapes, levels)]
    tab = _table(bands)
    if adjoint_of_inverse:
        _run("ext3db_inverse_adjoint", sfx, x, L.pdwt_ext3db_tmp_elems(V, Nz, Nr, Nc, f.hlen, levels),  # (the forward in mode zero: no frames)
             lambda fn, t: fn(C.c_void_p(x.data_ptr()), tab, V, Nz, Nr, Nc, levels, C.byref(f), t))
    else:
        _run("ext3db_forward", sfx, x, L.pdwt_ext3db_tmp_elems(V, Nz, Nr, Nc, f.hlen, levels),
             lambda fn, t: fn(C.c_void_p(x.data_ptr()), tab, V, Nz, Nr, Nc, levels, m, C.byref(f), t))
    return bands


def _idwt3(bands, shape, wname, mode=None):
    """mode None: the inverse; a mode: the adjoint of the forward transform"""
    bands, sfx, levels = _band_list(bands, 7, MAX_LEVELS_3D)
    f = _bank(wname, sfx)
    m = None if mode is None else _mode(mode)
    Nz, Nr, Nc = _shape3(shape)
    shapes = _geom3((Nz, Nr, Nc), f.hlen, levels)
    if bands[0].dim() < 3:
        raise ValueError("bands of shape (..., nz, nr, nc) are required")
    lead = tuple(bands[0].shape[:-3])
    _check_shapes(bands, lead, _table_shapes3(shapes, levels))
    V = _count(lead, (1 << 31) - 1, "volumes")
    L = N.hip()
    out = bands[0].new_empty(lead + (Nz, Nr, Nc))
    tab = _table(bands)
    if m is None:
        _run("ext3db_inverse", sfx, out, L.pdwt_ext3db_tmp_elems(V, Nz, Nr, Nc, f.hlen, levels),
             lambda fn, t: fn(C.c_void_p(out.data_ptr()), tab, V, Nz, Nr, Nc, levels, C.byref(f), t))
    else:
        _run("ext3db_forward_adjoint", sfx, out, L.pdwt_ext3db_adjoint_tmp_elems(V, Nz, Nr, Nc, f.hlen, levels),
             lambda fn, t: fn(C.c_void_p(out.data_ptr()), tab, V, Nz, Nr, Nc, levels, m, C.byref(f), t))
    return out


# ---- the bare adjoints -----------------------------------------------------------------------------------------------------------
def dwt2_adjoint(bands, shape, wname, mode="symmetric"):
    """W^T: the cotangents of ``dwt2``'s band list -> a tensor of shape (..., Nr, Nc); ``shape`` = (Nr, Nc)"""
    return _idwt2([b.detach() for b in _tensors(bands)], shape, wname, mode)


def idwt2_adjoint(x, wname, levels=1):
    """S^T: the cotangent of ``idwt2``'s image -> the band list of ``levels`` levels"""
    _sfx(x)
    return _dwt2(x.detach(), wname, levels, None, adjoint_of_inverse=True)


def dwt1_adjoint(bands, n, wname, mode="symmetric"):
    return _idwt1([b.detach() for b in _tensors(bands)], n, wname, mode)


def idwt1_adjoint(x, wname, levels=1):
    _sfx(x)
    return _dwt1(x.detach(), wname, levels, None, adjoint_of_inverse=True)


def dwt3_adjoint(bands, shape, wname, mode="symmetric"):
    """W^T: the cotangents of ``dwt3``'s band table -> a tensor of shape (..., Nz, Nr, Nc); ``shape`` = (Nz, Nr, Nc)"""
    return _idwt3([b.detach() for b in _tensors(bands)], shape, wname, mode)


def idwt3_adjoint(x, wname, levels=1):
    """S^T: the cotangent of ``idwt3``'s volume -> the band table of ``levels`` levels (the order of ``dwt3``)"""
    _sfx(x)
    return _dwt3(x.detach(), wname, levels, None, adjoint_of_inverse=True)


def _tensors(bands):
    if not isinstance(bands, (list, tuple)):
        raise ValueError("a list of band tensors is required")
    for b in bands:
        _sfx(b)
    return bands


# ---- autograd ----------------------------------------------------------------------------------------------------------------------
def _functions():
    """the six torch.autograd.Functions, made on first use (importing pdwt_amd does not import torch)"""
    global _fn
    if _fn is not None:
        return _fn
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class DWT2(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, wname, levels, mode):
            ctx.meta = (tuple(x.shape[-2:]), wname, mode)
            return tuple(_dwt2(x.detach(), wname, levels, mode))

        @staticmethod
        @once_differentiable
        def backward(ctx, *grads):
            shape, wname, mode = ctx.meta
            return _idwt2([g.contiguous() for g in grads], shape, wname, mode), None, None, None

    class IDWT2(torch.autograd.Function):
        @staticmethod
        def forward(ctx, shape, wname, *bands):
            ctx.meta = (wname, (len(bands) - 1) // 3)
            return _idwt2([b.detach() for b in bands], shape, wname)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad):
            wname, levels = ctx.meta
            return (None, None) + tuple(_dwt2(grad.contiguous(), wname, levels, None, adjoint_of_inverse=True))

    class DWT1(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, wname, levels, mode):
            ctx.meta = (int(x.shape[-1]), wname, mode)
            return tuple(_dwt1(x.detach(), wname, levels, mode))

        @staticmethod
        @once_differentiable
        def backward(ctx, *grads):
            n, wname, mode = ctx.meta
            return _idwt1([g.contiguous() for g in grads], n, wname, mode), None, None, None

    class IDWT1(torch.autograd.Function):
        @staticmethod
        def forward(ctx, n, wname, *bands):
            ctx.meta = (wname, len(bands) - 1)
            return _idwt1([b.detach() for b in bands], n, wname)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad):
            wname, levels = ctx.meta
            return (None, None) + tuple(_dwt1(grad.contiguous(), wname, levels, None, adjoint_of_inverse=True))

    class DWT3(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, wname, levels, mode):
            ctx.meta = (tuple(x.shape[-3:]), wname, mode)
            return tuple(_dwt3(x.detach(), wname, levels, mode))

        @staticmethod
        @once_differentiable
        def backward(ctx, *grads):
            shape, wname, mode = ctx.meta
            return _idwt3([g.contiguous() for g in grads], shape, wname, mode), None, None, None

    class IDWT3(torch.autograd.Function):
        @staticmethod
        def forward(ctx, shape, wname, *bands):
            ctx.meta = (wname, (len(bands) - 1) // 7)
            return _idwt3([b.detach() for b in bands], shape, wname)

        @staticmethod
        @once_differentiable
        def backward(ctx, grad):
            wname, levels = ctx.meta
            return (None, None) + tuple(_dwt3(grad.contiguous(), wname, levels, None, adjoint_of_inverse=True))

    _fn = {"dwt2": DWT2, "idwt2": IDWT2, "dwt1": DWT1, "idwt1": IDWT1, "dwt3": DWT3, "idwt3": IDWT3}
    return _fn


def dwt2(x, wname, levels=1, mode="symmetric"):
    """[A_L, H1, V1, D1, ..., H_L, V_L, D_L] of x (..., Nr, Nc): pywt.wavedec2(x, wname, mode, levels, axes=(-2, -1))"""
    _sfx(x)
    return list(_functions()["dwt2"].apply(x, wname, levels, mode))


def idwt2(bands, shape, wname):
    """the (..., Nr, Nc) tensor of ``shape`` = (Nr, Nc) from the band list of ``dwt2`` (no mode: the inverse needs no extension)"""
    return _functions()["idwt2"].apply(tuple(shape), wname, *_tensors(bands))


def dwt1(x, wname, levels=1, mode="symmetric"):
    """[A_L, D_1, ..., D_L] along the last axis of x (..., n): pywt.wavedec(x, wname, mode, levels, axis=-1)"""
    _sfx(x)
    return list(_functions()["dwt1"].apply(x, wname, levels, mode))


def idwt1(bands, n, wname):
    """the (..., n) tensor from the band list of ``dwt1``"""
    return _functions()["idwt1"].apply(n, wname, *_tensors(bands))


def dwt3(x, wname, levels=1, mode="symmetric"):
    """[A_L, the 7 details of level L, ..., the 7 details of level 1] of x (..., Nz, Nr, Nc), a level's details in the order aad, ada, add,
    daa, dad, dda, ddd (first letter: the z axis): the band table of ``BoundaryWavelets3D`` and the flattened ``pywt.wavedecn(x, wname, mode,
    levels, axes=(-3, -2, -1))``.  The COARSEST level comes first -- unlike ``dwt2``, whose details run from level 1 up.  ``levels`` is
    1 .. 13 and is not clamped."""
    _sfx(x)
    return list(_functions()["dwt3"].apply(x, wname, levels, mode))


def idwt3(bands, shape, wname):
    """the (..., Nz, Nr, Nc) tensor of ``shape`` = (Nz, Nr, Nc) from the band table of ``dwt3`` (no mode: the inverse needs no extension)"""
    return _functions()["idwt3"].apply(tuple(shape), wname, *_tensors(bands))
