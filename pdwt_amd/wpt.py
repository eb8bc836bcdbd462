"""Python views of the C++ wavelet packet classes: ``WaveletPackets`` (include/wpt.h), the 2-D transform -- the full quad-tree, in which
every band is decomposed again --, ``WaveletPackets1D`` (include/wpt1d.h), the full binary tree of every row of a batch, and
``WaveletPacketsImages`` (include/wpt_batch.h), the quad-tree of every image of a stack; all with best-basis selection.

A node is named by a path string with one letter per depth, the first level the most significant, or by a ``(depth, idx)`` pair.  2-D:
``a h v d`` = digits 0 1 2 3, ``"ahd"`` is node 7 of depth 3, node ``i`` of depth ``l`` has the children ``4i .. 4i+3``.  1-D: ``a d`` =
digits 0 1, ``"ad"`` is node 1 of depth 2, children ``2i`` and ``2i+1``.  ``""`` is the input.  The order is the natural (Paley) one;
``frequency_order`` gives the permutation to frequency order for the 1-D tree.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .wavelets import DeviceArray, W_CREATION_ERROR, W_FORWARD, W_INVERSE, W_THRESHOLD, _device_source, _sync_producer

MAX_LEVELS = 7
MAX_LEVELS_1D = 12
COSTS = {"l1": 0, "shannon": 1}
_DIGIT = {"a": 0, "h": 1, "v": 2, "d": 3}
_LETTERS = {4: _DIGIT, 2: {"a": 0, "d": 1}}


def path_to_index(path, arity=4):
    """(depth, idx) of the node a path string names; ``ValueError`` for a letter outside ``ahvd`` (``arity=2``: outside ``ad``)."""
    digit = _LETTERS[arity]
    idx = 0
    for ch in path:
        if ch not in digit:
            raise ValueError("bad letter %r in node path %r (%s)" % (ch, path, ", ".join(digit)))
        idx = arity * idx + digit[ch]
    return len(path), idx


def check_basis(nodes, levels, arity=4):
    """Sorted list of (depth, idx) if ``nodes`` is a basis of a tree of ``levels`` depths -- every root-to-leaf path meets exactly one
    of them -- else ``ValueError``.  Nodes may be paths or pairs.  ``arity``: children per node (4: the 2-D tree, 2: the 1-D tree)."""
    out, leaf = [], np.zeros(arity ** levels, dtype=bool)
    for nd in nodes:
        d, i = path_to_index(nd, arity) if isinstance(nd, str) else (int(nd[0]), int(nd[1]))
        if not (0 <= d <= levels and 0 <= i < arity ** d):
            raise ValueError("node %r is outside a tree of %d levels" % (nd, levels))
        span = arity ** (levels - d)
        if leaf[i * span:(i + 1) * span].any():
            raise ValueError("node %r overlaps another node of the basis" % (nd,))
        leaf[i * span:(i + 1) * span] = True
        out.append((d, i))
    if not leaf.all():
        raise ValueError("the basis is incomplete: some root-to-leaf paths meet no node")
    return sorted(out)


def frequency_order(depth):
    """int array ``f`` of 2^depth entries: ``f[r] = r ^ (r >> 1)`` is the natural index of the 1-D node of frequency rank ``r`` (Gray
    code; depth 2: ``aa, ad, dd, da``, PyWavelets' ``order='freq'``)."""
    depth = int(depth)
    if not 0 <= depth <= MAX_LEVELS_1D:
        raise ValueError("depth must be 0 .. %d" % MAX_LEVELS_1D)
    r = np.arange(2 ** depth)
    return r ^ (r >> 1)


class WaveletPackets2D:
    """WaveletPackets2D(img, wname, levels, dtype=None): ``img`` is a 2-D numpy array or a contiguous float32 / float64 device tensor
    (copied device to device, as ``Wavelets`` does).  Same state machine as ``Wavelets``; device memory about (levels + 1) images."""

    # what a subclass over another tree replaces: handle prefix, children per node, info struct, the two error texts that name the class
    _hpfx, _arity, _info_t = "pdwt_wpt_", 4, N.InfoWPT
    _err_shape = "WaveletPackets2D needs a 2-D image (Nr, Nc)"
    _err_alloc = "WaveletPackets2D allocation failed"

    def _fn(self, name):
        return getattr(self._L, self._hpfx + name)

    def __init__(self, img, wname, levels, dtype=None):
        N.require_gpu()
        dev = _device_source(img)
        if dev is not None:
            ptr, shape, dt = dev
            if dtype is not None and np.dtype(dtype) != dt:
                raise TypeError("dtype does not match the device tensor")
            _sync_producer()
            src, on_host, keep = C.c_void_p(ptr), 0, None
        else:
            img = np.asarray(img)
            dt = np.dtype(dtype or (img.dtype if img.dtype in (np.float32, np.float64) else np.float32))
            keep = np.ascontiguousarray(img, dtype=dt)
            shape, src, on_host = keep.shape, keep.ctypes.data_as(C.c_void_p), 1
        if len(shape) != 2:
            raise ValueError(self._err_shape)
        self.dtype, self.shape, self.wname = np.dtype(dt), tuple(int(v) for v in shape), wname
        self._L = N.host(self.dtype)
        self._ct = C.c_float if self.dtype == np.float32 else C.c_double
        self._h = self._fn("new")(src, self.shape[0], self.shape[1], wname.encode(), int(levels), on_host)
        del keep
        if not self._h:
            raise MemoryError(self._err_alloc)

    def close(self):
        if getattr(self, "_h", None):
            self._fn("delete")(self._h)
        self._h = None

    __del__ = close

    # -- introspection ---------------------------------------------------------------------
    @property
    def info(self):
        i = self._info_t()
        self._fn("info")(self._h, C.byref(i))
        return i

    @property
    def levels(self):
        return self.info.nlevels

    @property
    def state(self):
        return self._fn("state")(self._h)

    def node_shape(self, depth):
        r, c = C.c_int(), C.c_int()
        if self._fn("node_shape")(self._h, int(depth), C.byref(r), C.byref(c)) <= 0:
            raise IndexError(depth)
        return r.value, c.value

    def _node(self, node):
        d, i = path_to_index(node, self._arity) if isinstance(node, str) else (int(node[0]), int(node[1]))
        if not (0 <= d <= self.levels and 0 <= i < self._arity ** d):
            raise IndexError(node)
        return d, i

    def _need_coeffs(self, what):
        if self.state in (W_INVERSE, W_CREATION_ERROR):
            raise RuntimeError("%s refused (state=%d): the coefficients are not valid" % (what, self.state))

    # -- transforms ------------------------------------------------------------------------
    def forward(self):
        self._fn("forward")(self._h)

    def inverse(self):
        self._fn("inverse")(self._h)

    # -- data in and out -------------------------------------------------------------------
    def get_image(self):
        out = np.empty(self.shape, dtype=self.dtype)
        if self._fn("get_image")(self._h, out.ctypes.data_as(C.c_void_p)) != out.size:
            raise RuntimeError("get_image failed")
        return out

    def _upload(self, fn, arr, n, *args):
        dev = _device_source(arr)
        if dev is not None:
            if dev[2] != self.dtype or int(np.prod(dev[1])) != n:
                raise ValueError("device array of the wrong dtype or size")
            _sync_producer()
            return fn(self._h, C.c_void_p(dev[0]), *args, 1)
        a = np.ascontiguousarray(arr, dtype=self.dtype)
        if a.size != n:
            raise ValueError("array of the wrong size")
        return fn(self._h, a.ctypes.data_as(C.c_void_p), *args, 0)

    def set_image(self, img):
        self._upload(self._fn("set_image"), img, self.shape[0] * self.shape[1])

    def get_level(self, depth):
        """All nodes of ``depth`` as one array of shape (4^depth, nr, nc)."""
        self._need_coeffs("get_level")
        out = np.empty((4 ** int(depth),) + self.node_shape(depth), dtype=self.dtype)
        if self._fn("get_level")(self._h, out.ctypes.data_as(C.c_void_p), int(depth)) != out.size:
            raise RuntimeError("get_level(%d) failed (state=%d)" % (depth, self.state))
        return out

    def get_node(self, node):
        self._need_coeffs("get_node")
        d, i = self._node(node)
        out = np.empty(self.node_shape(d), dtype=self.dtype)
        if self._fn("get_node")(self._h, out.ctypes.data_as(C.c_void_p), d, i) != out.size:
            raise RuntimeError("get_node(%r) failed (state=%d)" % (node, self.state))
        return out

    def set_node(self, node, arr):
        """Overwrite one node (dense numpy array or device tensor of ``node_shape``); the state becomes W_THRESHOLD.  Needs the tree of a ``forward()``:
        refused (``RuntimeError``) before it and after ``inverse()``."""
        if self.state not in (W_FORWARD, W_THRESHOLD):
            raise RuntimeError("set_node refused (state=%d): run forward() first" % self.state)
        d, i = self._node(node)
        r, c = self.node_shape(d)
        if self._upload(self._fn("set_node"), arr, r * c, d, i) != r * c:
            raise RuntimeError("set_node(%r) failed (state=%d)" % (node, self.state))

    def node_int_ptr(self, node):
        d, i = self._node(node)
        return self._fn("node_int_ptr")(self._h, d, i)

    def node_view(self, node):
        """One node as a zero-copy DeviceArray (call ``sync()`` before a consumer on another stream reads it)."""
        d, _ = self._node(node)
        return DeviceArray(self, self.node_int_ptr(node), self.node_shape(d), self.dtype)

    def sync(self):
        return N.hip().pdwt_sync()

    # -- costs and bases -------------------------------------------------------------------
    def node_costs(self, cost="shannon"):
        """[float64 array of 4^depth costs for depth 0 .. levels]; ``"l1"``: sum |c|, ``"shannon"``: -sum c^2 ln c^2.  Depth 0 is the
        cost of the image.  One launch per depth; sums in double, combined in a fixed order."""
        if cost not in COSTS:
            raise ValueError("cost must be 'l1' or 'shannon'")
        out = []
        for d in range(self.levels + 1):
            c = np.empty(self._arity ** d, dtype=np.float64)
            if self._fn("node_costs")(self._h, d, COSTS[cost], c.ctypes.data_as(C.POINTER(C.c_double))) != 0:
                raise RuntimeError("node_costs refused (state=%d): the coefficients are not valid" % self.state)
            out.append(c)
        return out

    @property
    def basis(self):
        """The current basis as a sorted list of (depth, idx)."""
        n = self._fn("basis_size")(self._h)
        d, i = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))()
        self._fn("get_basis")(self._h, d, i)
        return [(d[k], i[k]) for k in range(n)]

    def best_basis(self, cost="shannon"):
        """Coifman-Wickerhauser search, bottom-up on the host over ``node_costs(cost)``: a parent is kept when its cost is <= the
        sum of its children's best costs (1-D: costs summed over the rows).  Installs the basis and returns it.  Needs the untouched tree of one forward()."""
        if cost not in COSTS:
            raise ValueError("cost must be 'l1' or 'shannon'")
        if self._fn("best_basis")(self._h, COSTS[cost]) < 1:
            raise RuntimeError("best_basis refused (state=%d): it needs the coefficients of forward(), unmodified" % self.state)
        return self.basis

    def set_basis(self, nodes):
        """Install a basis: paths or (depth, idx) pairs that partition the tree (``ValueError`` otherwise)."""
        b = check_basis(nodes, self.levels, self._arity)
        if self.state == W_THRESHOLD:
            raise RuntimeError("set_basis refused (state=%d): the coefficients were modified, the tree is no longer one transform" % self.state)
        n = len(b)
        d, i = (C.c_int * n)(*[v[0] for v in b]), (C.c_int * n)(*[v[1] for v in b])
        if self._fn("set_basis")(self._h, d, i, n) != 0:
            raise RuntimeError("set_basis failed (state=%d)" % self.state)

    # -- thresholds, norms, statistics over the basis --------------------------------------
    def soft_threshold(self, beta, do_thresh_appcoeffs=0):
        """In place on the nodes of the current basis; the all-``a`` node only when ``do_thresh_appcoeffs``."""
        self._need_coeffs("soft_threshold")
        self._fn("soft_threshold")(self._h, self._ct(beta), int(do_thresh_appcoeffs))

    def hard_threshold(self, beta, do_thresh_appcoeffs=0):
        self._need_coeffs("hard_threshold")
        self._fn("hard_threshold")(self._h, self._ct(beta), int(do_thresh_appcoeffs))

    def norm1(self):
        """Sum of |c| over the nodes of the basis, in double."""
        v = float(self._fn("norm1")(self._h))
        if v < 0:
            raise RuntimeError("norm1 refused (state=%d): the coefficients are not valid" % self.state)
        return v

    def node_stats(self, depth):
        """{sum_abs, sum_sq, max_abs: float64 arrays of 4^depth (1-D: 2^depth, over all rows)} of the nodes of ``depth``, one batched launch."""
        n = self._arity ** int(depth)
        self.node_shape(depth)
        out = (N.BandStats * n)()
        if self._fn("node_stats")(self._h, int(depth), out) != 0:
            raise RuntimeError("node_stats refused (state=%d): the coefficients are not valid" % self.state)
        a = np.frombuffer(out, dtype=np.float64).reshape(n, 5)
        return {"sum_abs": a[:, 1].copy(), "sum_sq": a[:, 2].copy(), "max_abs": a[:, 3].copy()}

    def estimate_sigma(self):
        """Noise level from the finest diagonal (1-D: detail) node: median |node "d"| / 0.6744897501960817 (1-D: over the whole batch)."""
        s = float(self._fn("estimate_sigma")(self._h))
        if s < 0:
            raise RuntimeError("estimate_sigma refused (state=%d): the coefficients are not valid" % self.state)
        return s


class PitchedDeviceArray(DeviceArray):
    """Zero-copy view of a 2-D strided run of device memory: rows of ``shape[1]`` elements, ``pitch`` ELEMENTS apart (a node of
    ``WaveletPackets1D``).  ``__cuda_array_interface__`` carries the strides, so ``torch.as_tensor(view, device="cuda")`` is a strided
    tensor over the node itself."""

    def __init__(self, owner, ptr, shape, dtype, pitch):
        super().__init__(owner, ptr, shape, dtype)
        self.pitch = int(pitch)

    @property
    def __cuda_array_interface__(self):
        isz = self.dtype.itemsize
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False), "version": 2, "strides": (self.pitch * isz, isz)}

    def numpy(self):
        out = np.empty(self.shape, dtype=self.dtype)
        w = self.shape[1] * self.dtype.itemsize
        if N.hip().pdwt_memcpy2d(out.ctypes.data_as(C.c_void_p), w, C.c_void_p(self.ptr), self.pitch * self.dtype.itemsize, w, self.shape[0], 1) != 0:
            raise RuntimeError("device-to-host copy failed")
        return out


class WaveletPackets1D(WaveletPackets2D):
    """WaveletPackets1D(rows, wname, levels, dtype=None): the packet tree of every row of a 2-D batch ``(Nr, Nc)`` -- a numpy array or a
    contiguous float32 / float64 device tensor (copied device to device) -- ``pywt.WaveletPacket(mode='periodization')`` per row.  Depth
    ``l`` is stored as ``(Nr, 2^l, n_l)``; one basis serves the whole batch.  Same methods and state machine as ``WaveletPackets2D``;
    paths are over ``ad``; ``node_shape(depth)`` is ``(Nr, n_depth)``.  Device memory about (levels + 1) batches.  ``fused``: the whole
    tree of a row runs in one launch.  Only what the rows change is written here."""

    _hpfx, _arity, _info_t = "pdwt_wp1h_", 2, N.InfoWPT1
    _err_shape = "WaveletPackets1D needs a 2-D batch of rows (Nr, Nc)"
    _err_alloc = "WaveletPackets1D allocation failed"

    @property
    def fused(self):
        return bool(self._fn("fused")(self._h))

    def get_level(self, depth, order="natural"):
        """All nodes of ``depth`` as one array of shape (Nr, 2^depth, n_depth); ``order="freq"``: the nodes in frequency order."""
        if order not in ("natural", "freq"):
            raise ValueError("order must be 'natural' or 'freq'")
        self._need_coeffs("get_level")
        r, n = self.node_shape(depth)
        out = np.empty((r, 2 ** int(depth), n), dtype=self.dtype)
        if self._fn("get_level")(self._h, out.ctypes.data_as(C.c_void_p), int(depth)) != out.size:
            raise RuntimeError("get_level(%d) failed (state=%d)" % (depth, self.state))
        return out if order == "natural" else np.ascontiguousarray(out[:, frequency_order(depth)])

    def node_int_ptr(self, node):
        """Device address of row 0 of the node; see ``node_pitch``."""
        d, i = self._node(node)
        return self._fn("node_int_ptr")(self._h, d, i, None)

    def node_pitch(self, node):
        """Distance between consecutive rows of the node, in elements: 2^depth * n_depth."""
        d, i = self._node(node)
        p = C.c_longlong()
        self._fn("node_int_ptr")(self._h, d, i, C.byref(p))
        return p.value

    def node_view(self, node):
        """One node as a zero-copy strided ``PitchedDeviceArray`` (call ``sync()`` before a consumer on another stream reads it)."""
        d, _ = self._node(node)
        return PitchedDeviceArray(self, self.node_int_ptr(node), self.node_shape(d), self.dtype, self.node_pitch(node))

    def node_costs(self, cost="shannon", per_row=False):
        """[float64 array of 2^depth costs for depth 0 .. levels], summed over the rows in row order; ``"l1"``: sum |c|, ``"shannon"``:
        -sum c^2 ln c^2.  ``per_row=True``: arrays of shape (Nr, 2^depth) instead, what a basis per row would be chosen from.  One
        launch per depth; sums in double, combined in a fixed order."""
        if cost not in COSTS:
            raise ValueError("cost must be 'l1' or 'shannon'")
        out = []
        for d in range(self.levels + 1):
            c = np.empty(2 ** d, dtype=np.float64)
            pr = np.empty((self.shape[0], 2 ** d), dtype=np.float64)
            if self._fn("node_costs")(self._h, d, COSTS[cost], c.ctypes.data_as(C.POINTER(C.c_double)), pr.ctypes.data_as(C.POINTER(C.c_double))) != 0:
                raise RuntimeError("node_costs refused (state=%d): the coefficients are not valid" % self.state)
            out.append(pr if per_row else c)
        return out


class StackDeviceArray(PitchedDeviceArray):
    """Zero-copy view of a stack of B contiguous (nr, nc) blocks ``pitch`` ELEMENTS apart (a node of ``WaveletPacketBatch`` across the
    images).  ``__cuda_array_interface__`` carries the strides."""

    @property
    def __cuda_array_interface__(self):
        isz = self.dtype.itemsize
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False), "version": 2,
                "strides": (self.pitch * isz, self.shape[2] * isz, isz)}

    def numpy(self):
        out = np.empty(self.shape, dtype=self.dtype)
        w = self.shape[1] * self.shape[2] * self.dtype.itemsize
        if N.hip().pdwt_memcpy2d(out.ctypes.data_as(C.c_void_p), w, C.c_void_p(self.ptr), self.pitch * self.dtype.itemsize, w, self.shape[0], 1) != 0:
            raise RuntimeError("device-to-host copy failed")
        return out


class WaveletPacketBatch(WaveletPackets2D):
    """WaveletPacketBatch(imgs, wname, levels, dtype=None, allow_fused=True): the packet quad-tree of every image of a stack ``(B, Nr, Nc)``
    -- a numpy array or a contiguous float32 / float64 device tensor (copied device to device) -- each image exactly as
    ``WaveletPackets2D`` would transform it (the same bits).  Depth ``l`` is stored as ``(B, 4^l, nr_l, nc_l)``; ONE basis serves the
    whole batch, chosen by ``best_basis`` from the costs summed over the images.  Same methods and state machine as
    ``WaveletPackets2D``; ``node_shape(depth)`` is the shape of one node of one image.  ``fused``: the whole tree of an image runs in the
    LDS of one workgroup, one launch per direction (``allow_fused=False``: depth by depth over the forest of all images).  Device
    memory about (levels + 1) batches.  Only what the batch changes is written here."""

    _hpfx, _arity, _info_t = "pdwt_wpbh_", 4, N.InfoWPTB
    _err_shape = "WaveletPacketBatch needs a stack of images (B, Nr, Nc)"
    _err_alloc = "WaveletPacketBatch allocation failed"

    def __init__(self, imgs, wname, levels, dtype=None, allow_fused=True):
        N.require_gpu()
        dev = _device_source(imgs)
        if dev is not None:
            ptr, shape, dt = dev
            if dtype is not None and np.dtype(dtype) != dt:
                raise TypeError("dtype does not match the device tensor")
            _sync_producer()
            src, on_host, keep = C.c_void_p(ptr), 0, None
        else:
            imgs = np.asarray(imgs)
            dt = np.dtype(dtype or (imgs.dtype if imgs.dtype in (np.float32, np.float64) else np.float32))
            keep = np.ascontiguousarray(imgs, dtype=dt)
            shape, src, on_host = keep.shape, keep.ctypes.data_as(C.c_void_p), 1
        if len(shape) != 3:
            raise ValueError(self._err_shape)
        self.dtype, self.shape, self.wname = np.dtype(dt), tuple(int(v) for v in shape), wname
        self._L = N.host(self.dtype)
        self._ct = C.c_float if self.dtype == np.float32 else C.c_double
        self._h = self._fn("new")(src, self.shape[0], self.shape[1], self.shape[2], wname.encode(), int(levels), on_host, 1 if allow_fused else 0)
        del keep
        if not self._h:
            raise MemoryError(self._err_alloc)

    @property
    def fused(self):
        return bool(self._fn("fused")(self._h))

    def set_image(self, imgs):
        """Replace the whole stack ``(B, Nr, Nc)``."""
        self._upload(self._fn("set_image"), imgs, self.shape[0] * self.shape[1] * self.shape[2])

    def get_level(self, depth):
        """All nodes of ``depth`` as one array of shape (B, 4^depth, nr, nc)."""
        self._need_coeffs("get_level")
        out = np.empty((self.shape[0], 4 ** int(depth)) + self.node_shape(depth), dtype=self.dtype)
        if self._fn("get_level")(self._h, out.ctypes.data_as(C.c_void_p), int(depth)) != out.size:
            raise RuntimeError("get_level(%d) failed (state=%d)" % (depth, self.state))
        return out

    def get_node(self, node):
        """One node across the images: shape (B, nr, nc)."""
        self._need_coeffs("get_node")
        d, i = self._node(node)
        out = np.empty((self.shape[0],) + self.node_shape(d), dtype=self.dtype)
        if self._fn("get_node")(self._h, out.ctypes.data_as(C.c_void_p), d, i) != out.size:
            raise RuntimeError("get_node(%r) failed (state=%d)" % (node, self.state))
        return out

    def set_node(self, node, arr):
        """Overwrite one node in every image (a ``(B, nr, nc)`` numpy array or device tensor); the state becomes W_THRESHOLD."""
        if self.state not in (W_FORWARD, W_THRESHOLD):
            raise RuntimeError("set_node refused (state=%d): run forward() first" % self.state)
        d, i = self._node(node)
        r, c = self.node_shape(d)
        n = self.shape[0] * r * c
        if self._upload(self._fn("set_node"), arr, n, d, i) != n:
            raise RuntimeError("set_node(%r) failed (state=%d)" % (node, self.state))

    def node_int_ptr(self, node):
        """Device address of the node of image 0; see ``node_pitch``."""
        d, i = self._node(node)
        return self._fn("node_int_ptr")(self._h, d, i, None)

    def node_pitch(self, node):
        """Distance between the node of consecutive images, in elements: 4^depth * nr * nc."""
        d, i = self._node(node)
        p = C.c_longlong()
        self._fn("node_int_ptr")(self._h, d, i, C.byref(p))
        return p.value

    def node_view(self, node):
        """One node across the images as a zero-copy strided ``StackDeviceArray`` (B, nr, nc) (call ``sync()`` before a consumer on
        another stream reads it)."""
        d, _ = self._node(node)
        return StackDeviceArray(self, self.node_int_ptr(node), (self.shape[0],) + self.node_shape(d), self.dtype, self.node_pitch(node))

    def level_view(self, depth):
        """A whole depth as a zero-copy contiguous DeviceArray (B, 4^depth, nr, nc); depth 0: the images (B, 1, Nr, Nc)."""
        return DeviceArray(self, self._fn("node_int_ptr")(self._h, int(depth), 0, None), (self.shape[0], 4 ** int(depth)) + self.node_shape(depth), self.dtype)

    def node_costs(self, cost="shannon", per_image=False):
        """[float64 array of 4^depth costs for depth 0 .. levels], summed over the images in image order; ``per_image=True``: arrays of
        shape (B, 4^depth) instead.  Sums in double, combined in a fixed order: two runs give the same bits."""
        if cost not in COSTS:
            raise ValueError("cost must be 'l1' or 'shannon'")
        out = []
        for d in range(self.levels + 1):
            c = np.empty(4 ** d, dtype=np.float64)
            pi = np.empty((self.shape[0], 4 ** d), dtype=np.float64)
            if self._fn("node_costs")(self._h, d, COSTS[cost], pi.ctypes.data_as(C.POINTER(C.c_double)), c.ctypes.data_as(C.POINTER(C.c_double))) != 0:
                raise RuntimeError("node_costs refused (state=%d): the coefficients are not valid" % self.state)
            out.append(pi if per_image else c)
        return out

    def node_stats(self, depth):
        """{sum_abs, sum_sq, max_abs: float64 arrays (B, 4^depth)} of every node of ``depth`` of every image, one batched launch."""
        n = self.shape[0] * 4 ** int(depth)
        self.node_shape(depth)
        out = (N.BandStats * n)()
        if self._fn("node_stats")(self._h, int(depth), out) != 0:
            raise RuntimeError("node_stats refused (state=%d): the coefficients are not valid" % self.state)
        a = np.frombuffer(out, dtype=np.float64).reshape(self.shape[0], 4 ** int(depth), 5)
        return {"sum_abs": a[..., 1].copy(), "sum_sq": a[..., 2].copy(), "max_abs": a[..., 3].copy()}

    def images_norm1(self):
        """Sum of |c| over the nodes of the basis, per image: float64 array (B,)."""
        out = np.empty(self.shape[0], dtype=np.float64)
        if self._fn("images_norm1")(self._h, out.ctypes.data_as(C.POINTER(C.c_double))) != 0:
            raise RuntimeError("images_norm1 refused (state=%d): the coefficients are not valid" % self.state)
        return out

    def images_estimate_sigma(self):
        """Noise level of each image from its own node ``"d"``: float64 array (B,).  ``estimate_sigma()`` pools all images."""
        out = np.empty(self.shape[0], dtype=np.float64)
        if self._fn("images_estimate_sigma")(self._h, out.ctypes.data_as(C.POINTER(C.c_double))) != 0:
            raise RuntimeError("images_estimate_sigma refused (state=%d): the coefficients are not valid" % self.state)
        return out
