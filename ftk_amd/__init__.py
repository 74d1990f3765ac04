"""ftk_amd -- MI355X-native critical-point space-time simplex sweep behind FTK's tracker API.

The product is the shared library ftk_amd/libftkx.so (HIP kernels for gfx950 + C ABI `ftkx_*`, see include/ftkx.h, and the C++
tracker of include/ftkx_tracker.hh).  This package is the Python plumbing over that C ABI, mirroring the reference's tracker
interface (include/ftk/filters/critical_point_tracker_{2d,3d}_regular.hh; python/pyftk.cpp:93-142)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (CP_DTYPE, FORMAT_BINARY, FORMAT_JSON, FORMAT_TEXT, SCOPE_BOTH, SCOPE_INTERVAL, SCOPE_ORDINAL, SOURCE_DERIVED, SOURCE_GIVEN, SOURCE_NONE,  # noqa: F401
                   TAG_EXACT64, TAG_REFERENCE, TAG_WORK_INDEX, FtkxError, Options, Stats)
from ._lib import DTYPE_BF16, DTYPE_F16, DTYPE_F32, DTYPE_F64, DTYPE_I8, DTYPE_I16, DTYPE_I32, DTYPE_U8, DTYPE_U16, DTYPE_U32  # noqa: F401

__all__ = ["trace_curves", "pass2", "trace_and_post_process", "post_process", "post_process_curves", "TrajectorySet", "write_critical_points", "read_critical_points",
           "write_traced_critical_points", "read_traced_critical_points", "Context", "CriticalPointTracker2DRegular", "CriticalPointTracker3DRegular", "extract_cp2dt", "extract_cp3dt",
           "scaling_factor", "gaussian_kernel", "gaussian_kernel1d", "CP_DTYPE", "FtkxError"]


def _ptr(a):
    """host numpy array / torch tensor / raw int -> (address, keepalive, on_device, f32).  A float32 array or tensor is kept as it is (f32
    True: it goes to the library's *_f32 entries, 4 bytes per value, and is widened on the device); a raw int is taken for float64"""
    if a is None:
        return None, None, 0, False
    if isinstance(a, int):
        return a, None, 1, False
    if hasattr(a, "data_ptr"):          # torch tensor (device memory is torch's job: plumbing, not the product)
        if a.dtype.is_floating_point and a.element_size() not in (4, 8):
            raise TypeError("fields must be float64 or float32")
        a = a.contiguous()
        return a.data_ptr(), a, 1 if a.is_cuda else 0, bool(a.dtype.is_floating_point and a.element_size() == 4)
    if isinstance(a, np.ndarray) and a.dtype == np.float32:
        a = np.ascontiguousarray(a)
        return a.ctypes.data, a, 0, True
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.ctypes.data, a, 0, False


_NUMPY_DTYPES = {np.dtype(np.float64): DTYPE_F64, np.dtype(np.float32): DTYPE_F32, np.dtype(np.float16): DTYPE_F16, np.dtype(np.uint8): DTYPE_U8, np.dtype(np.int8): DTYPE_I8,
                 np.dtype(np.uint16): DTYPE_U16, np.dtype(np.int16): DTYPE_I16, np.dtype(np.uint32): DTYPE_U32, np.dtype(np.int32): DTYPE_I32}
_TORCH_DTYPES = {"torch.float64": DTYPE_F64, "torch.float32": DTYPE_F32, "torch.float16": DTYPE_F16, "torch.bfloat16": DTYPE_BF16, "torch.uint8": DTYPE_U8, "torch.int8": DTYPE_I8,
                 "torch.uint16": DTYPE_U16, "torch.int16": DTYPE_I16, "torch.uint32": DTYPE_U32, "torch.int32": DTYPE_I32}


def _ptr_typed(a):
    """keep_dtype=True: host numpy array / torch tensor / raw int -> (address, the array itself, on_device, DTYPE_*).  The array goes to the
    library's typed entries with the element type it has -- float16, bfloat16 (torch), 8- / 16- / 32-bit integers, float32, float64 -- and
    is widened on the device; nothing is converted on the host.  Any other element type (64-bit integers, bool, complex, a byte order that
    is not the machine's) raises TypeError before the library is called.  A raw int is taken for float64"""
    if a is None:
        return None, None, 0, None
    if isinstance(a, int):
        return a, None, 1, DTYPE_F64
    if hasattr(a, "data_ptr"):
        dt = _TORCH_DTYPES.get(str(a.dtype))
        if dt is None:
            raise TypeError(f"keep_dtype: {a.dtype} is not taken (float64, float32, float16, bfloat16, and integers of 8, 16 or 32 bits)")
        a = a.contiguous()
        return a.data_ptr(), a, 1 if a.is_cuda else 0, dt
    if not isinstance(a, np.ndarray):
        raise TypeError("keep_dtype: a numpy array or a torch tensor")
    dt = _NUMPY_DTYPES.get(a.dtype) if a.dtype.isnative else None
    if dt is None:
        raise TypeError(f"keep_dtype: {a.dtype} is not taken (float64, float32, float16, and integers of 8, 16 or 32 bits)")
    a = np.ascontiguousarray(a)
    return a.ctypes.data, a, 0, dt


def _ptr_any(a, keep_dtype):
    """_ptr, or _ptr_typed where keep_dtype is set -> (address, keepalive, on_device, DTYPE_*)"""
    if keep_dtype:
        return _ptr_typed(a)
    p, k, d, f32 = _ptr(a)
    return p, k, d, None if p is None else DTYPE_F32 if f32 else DTYPE_F64


def _one_dtype(*dtypes):
    """the arrays of one push (those that are given) share one element type -> which"""
    kinds = {d for d in dtypes if d is not None}
    if len(kinds) > 1:
        if kinds <= {DTYPE_F32, DTYPE_F64}:
            raise TypeError("the arrays of one push must all be float32 or all float64")
        raise TypeError("the arrays of one push must share one element type")
    return kinds.pop() if kinds else DTYPE_F64


def _same_type(*f32):
    """the arrays of one push (those that are given) are all float32 or all float64 -> which"""
    kinds = {bool(f) for f in f32 if f is not None}
    if len(kinds) > 1:
        raise TypeError("the arrays of one push must all be float32 or all float64")
    return bool(kinds and kinds.pop())


def _planes(planes):
    """a vector snapshot as component planes -> (ctypes array of nc addresses, nc, keepalive, on_device, f32).  planes: a sequence of nc numpy
    arrays / torch tensors of one dtype (float32 or float64) and one size, each contiguous; or ONE contiguous array / tensor of shape
    (nc, ...), whose nc leading slices are the planes.  Nothing is copied: what is not contiguous is refused."""
    whole = planes if isinstance(planes, np.ndarray) or hasattr(planes, "data_ptr") else None
    if whole is not None:
        if whole.ndim < 2:
            raise ValueError("planes: one array of shape (nc, ...), or a sequence of nc arrays")
        seq = [whole[k] for k in range(whole.shape[0])]
    else:
        seq = list(planes)
    if not seq:
        raise ValueError("planes: no components")
    addrs, kinds, devs, sizes = [], set(), set(), set()
    for a in seq:
        if hasattr(a, "data_ptr"):
            size = a.element_size() if a.dtype.is_floating_point else 0
            contiguous, dev, addr, n = a.is_contiguous(), bool(a.is_cuda), a.data_ptr(), a.numel()
        elif isinstance(a, np.ndarray):
            size = a.dtype.itemsize if a.dtype.kind == "f" else 0
            contiguous, dev, addr, n = a.flags.c_contiguous, False, a.ctypes.data, a.size
        else:
            raise TypeError("planes must be numpy arrays or torch tensors")
        if size not in (4, 8):
            raise TypeError("planes must be float64 or float32")
        if not contiguous:
            raise ValueError("every plane must be contiguous")
        addrs.append(addr); kinds.add(size); devs.add(dev); sizes.add(n)
    if len(kinds) > 1:
        raise TypeError("the planes of one push must all be float32 or all float64")
    if len(devs) > 1:
        raise ValueError("the planes of one push must all be host arrays or all device tensors")
    if len(sizes) > 1:
        raise ValueError("the planes of one push must have one size")
    return (C.c_void_p * len(addrs))(*addrs), len(addrs), (seq, whole), 1 if devs.pop() else 0, kinds.pop() == 4


def default_options(**kw):
    o = Options()
    _lib.load().ftkx_default_options(C.byref(o))
    for k, v in kw.items():
        if k == "coords_bounds":
            o.coords_mode = 1
            for i, b in enumerate(v):
                o.coords_bounds[i] = float(b)
        else:
            setattr(o, k, int(v))
    return o


def scaling_factor(resolution):
    nb = C.c_int()
    f = _lib.load().ftkx_scaling_factor(float(resolution), C.byref(nb))
    return int(f), nb.value


def gaussian_kernel(nd, sigma, ksize):
    """ftkx_gaussian_kernel: the reference's gaussian_kernel2D / 3D weights (host), shape (ksize,) * nd with x last"""
    w = np.zeros(max(1, int(ksize)) ** nd if nd in (2, 3) else 1, dtype=np.float64)
    _lib.check(_lib.load().ftkx_gaussian_kernel(int(nd), float(sigma), int(ksize), w.ctypes.data))
    return w.reshape((int(ksize),) * nd)


def gaussian_kernel1d(sigma, ksize):
    """ftkx_gaussian_kernel1d: the weights of the reference's temporal filter (gaussian_kernel; host), ksize doubles"""
    w = np.zeros(max(1, int(ksize)), dtype=np.float64)
    _lib.check(_lib.load().ftkx_gaussian_kernel1d(float(sigma), int(ksize), w.ctypes.data))
    return w


class Context:
    """ftkx_ctx: slices resident in HBM + sweeps (include/ftkx.h)."""

    def __init__(self, nd, device_id=0):
        self._L = _lib.load()
        self.nd = nd
        self._h = C.c_void_p()
        _lib.check(self._L.ftkx_create(C.byref(self._h), nd, device_id))
        self._keep = {}
        self._keep_aux = {}
        self._smoothing = False
        self._vsmoothing = False
        self._perturbing = False
        self._clamping = False

    def close(self):
        if self._h:
            self._L.ftkx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        _lib.check(rc, self._h)

    def set_stream(self, stream_ptr):
        self._ck(self._L.ftkx_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_options(self, **kw):
        self._opt = default_options(**kw)
        self._ck(self._L.ftkx_set_options(self._h, C.byref(self._opt)))

    def set_coords_rectilinear(self, arrays):
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays] + [None] * (3 - len(arrays))
        args = []
        for a in arrs:
            args += [a.ctypes.data if a is not None else None, len(a) if a is not None else 0]
        self._ck(self._L.ftkx_set_coords_rectilinear(self._h, *args))

    def set_coords_explicit(self, coords):
        e = np.ascontiguousarray(coords, dtype=np.float64)
        self._ck(self._L.ftkx_set_coords_explicit(self._h, e.ctypes.data, e.shape[-1], e.shape[-2], e.shape[-3]))

    def set_mesh(self, domain, core, ext):
        """each = (starts, sizes), spatial axes only (x, y[, z])"""
        args = []
        for st, sz in (domain, core, ext):
            args += [_lib.ll(st), _lib.ll(sz, fill=1)]
        self._ck(self._L.ftkx_set_mesh(self._h, *args))
        self._n_vertices = int(np.prod([int(v) for v in ext[1]][:self.nd], dtype=np.int64))
        self._keep_aux = {}

    def set_spatial_smoothing(self, sigma, ksize=3):
        """ftkx_set_spatial_smoothing: scalar slices pushed from now on are conv_gaussian(S, sigma, ksize, ksize // 2); ksize 0: off"""
        rc = self._L.ftkx_set_spatial_smoothing(self._h, float(sigma), int(ksize))
        self._ck(rc)                                   # (raises: a refused setting leaves the context, and this flag, as they were)
        self._smoothing = int(ksize) != 0

    def set_vector_smoothing(self, sigma, ksize=3):
        """ftkx_set_vector_smoothing: vector snapshots pushed from now on (push_slice, push_slice_planar, temporal_push with a vector,
        temporal_push_planar) have every component smoothed as the scalar field it is -- conv_gaussian(component, sigma, ksize, ksize // 2),
        one kernel for the whole array; J or S beside V is refused while it is on.  A setting of its own beside set_spatial_smoothing;
        ksize 0: off"""
        self._ck(self._L.ftkx_set_vector_smoothing(self._h, float(sigma), int(ksize)))
        self._vsmoothing = int(ksize) != 0

    def set_perturbation(self, sigma, seed=0):
        """ftkx_set_perturbation: every snapshot pushed from now on gets sigma * N(0, 1) noise added on the device, the noise of element e of
        timestep t being a function of (seed, t, e) alone; sigma 0: off"""
        self._ck(self._L.ftkx_set_perturbation(self._h, float(sigma), int(seed)))
        self._perturbing = float(sigma) > 0

    def set_clamp(self, lo=None, hi=None):
        """ftkx_set_clamp: every snapshot pushed from now on becomes min(max(lo, x), hi) on the device (behind the perturbation); no bounds: off"""
        on = lo is not None or hi is not None
        if on and (lo is None or hi is None):
            raise ValueError("set_clamp: both bounds, or none")
        self._ck(self._L.ftkx_set_clamp(self._h, int(on), float(lo) if on else 0.0, float(hi) if on else 0.0))
        self._clamping = on

    def adjust(self, src_ptr, count, dst_ptr, sigma=0.0, seed=0, t=0, clamp=None, f32=False):
        """ftkx_adjust / ftkx_adjust_f32 on device pointers: dst[e] = clamp(double(src[e]) + sigma * z(seed, t, e)); clamp: (lo, hi) or None;
        dst_ptr == src_ptr is allowed for doubles"""
        lo, hi = clamp if clamp is not None else (0.0, 0.0)
        self._ck((self._L.ftkx_adjust_f32 if f32 else self._L.ftkx_adjust)(self._h, src_ptr, int(count), float(sigma), int(seed), int(t), int(clamp is not None), float(lo), float(hi), dst_ptr))

    def debug_adjust_relaunch(self, src_ptr, count, dst_ptr, reps, sigma=0.0, seed=0, t=0, clamp=None, f32=False):
        """profiling aid: the adjust kernel `reps` times back to back -> device ms per launch (HIP events)"""
        lo, hi = clamp if clamp is not None else (0.0, 0.0)
        ms = (C.c_double * int(reps))()
        self._ck(self._L.ftkx_debug_adjust_relaunch(self._h, src_ptr, int(bool(f32)), int(count), float(sigma), int(seed), int(t), int(clamp is not None), float(lo), float(hi), dst_ptr,
                                                    int(reps), ms))
        return list(ms)

    def adjust_counts(self):
        """(from_float, in_place, out_of_place): snapshots pushed into this context that went through the adjust kernel, by its kind"""
        a = C.c_ulonglong(0); b = C.c_ulonglong(0); c = C.c_ulonglong(0)
        self._ck(self._L.ftkx_debug_adjust_counts(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def set_temporal_smoothing(self, sigma, ksize=5, t0=0):
        """ftkx_set_temporal_smoothing: a series of raw snapshots for temporal_push starts, its first emission being timestep t0; ksize 0: off"""
        self._ck(self._L.ftkx_set_temporal_smoothing(self._h, float(sigma), int(ksize), int(t0)))

    def temporal_push(self, A, is_vector=False, on_device=None, keep_dtype=False):
        """ftkx_temporal_push: one raw snapshot (host array or device tensor; always copied) -> the timestep of the smoothed slice that became
        resident, or -1.  on_device and keep_dtype as in push_scalar_slice"""
        p, k, d, dt = _ptr_any(A, keep_dtype)
        f32 = dt == DTYPE_F32
        if on_device is not None:
            if int(on_device) not in (0, 1, 2) or (int(on_device) != 0) != bool(d):
                raise ValueError("on_device: 0 for a host array, 1 or 2 for a device tensor")
            d = int(on_device)
        t = C.c_int(-1)
        if dt is not None and dt > DTYPE_F32:
            self._ck(self._L.ftkx_temporal_push_typed(self._h, p, dt, int(bool(is_vector)), d, C.byref(t)))
        else:
            self._ck((self._L.ftkx_temporal_push_f32 if f32 else self._L.ftkx_temporal_push)(self._h, p, int(bool(is_vector)), d, C.byref(t)))
        if t.value >= 0:
            self._keep[t.value] = None
        return t.value

    def temporal_flush(self):
        """ftkx_temporal_flush: one finishing step -> the timestep of the trailing slice that became resident, or -1 when the series is over"""
        t = C.c_int(-1)
        self._ck(self._L.ftkx_temporal_flush(self._h, C.byref(t)))
        if t.value >= 0:
            self._keep[t.value] = None
        return t.value

    def _temporal_args(self, arrays, weights):
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if len(arrays) != w.size:
            raise ValueError("temporal_combine: one weight per array")
        return (C.c_void_p * len(arrays))(*[int(a) for a in arrays]), w

    def temporal_combine(self, array_ptrs, weights, count, out_ptr):
        """ftkx_temporal_combine on device pointers (repeats allowed): out[e] = w[0] * a0[e] + w[1] * a1[e] + ..., every step rounded"""
        ptrs, w = self._temporal_args(array_ptrs, weights)
        self._ck(self._L.ftkx_temporal_combine(self._h, ptrs, w.size, w.ctypes.data, int(count), out_ptr))

    def debug_temporal_relaunch(self, array_ptrs, weights, count, out_ptr, reps):
        """profiling aid: the temporal kernel `reps` times back to back -> device ms per launch (HIP events)"""
        ptrs, w = self._temporal_args(array_ptrs, weights)
        ms = (C.c_double * int(reps))()
        self._ck(self._L.ftkx_debug_temporal_relaunch(self._h, ptrs, w.size, w.ctypes.data, int(count), out_ptr, int(reps), ms))
        return list(ms)

    def push_slice(self, t, V, J=None, S=None, keep_dtype=False):
        """keep_dtype as in push_scalar_slice; V, J and S share one element type"""
        pv, kv, dv, fv = _ptr_any(V, keep_dtype); pj, kj, dj, fj = _ptr_any(J, keep_dtype); ps, ks, ds, fs = _ptr_any(S, keep_dtype)
        devs = {d for p, d in ((pv, dv), (pj, dj), (ps, ds)) if p is not None}
        if len(devs) != 1:
            raise ValueError("V, J, S must all be host arrays or all device tensors")
        on_dev = devs.pop()
        dt = _one_dtype(fv, fj, fs)
        f32 = dt == DTYPE_F32
        if dt > DTYPE_F32:
            self._ck(self._L.ftkx_push_slice_typed(self._h, t, pv, pj, ps, dt, on_dev))
        else:
            self._ck((self._L.ftkx_push_slice_f32 if f32 else self._L.ftkx_push_slice)(self._h, t, pv, pj, ps, on_dev))
        owned = dt != DTYPE_F64 or self._perturbing or self._clamping or self._vsmoothing
        self._keep[t] = (kv, kj, ks) if on_dev and not owned else None       # (float32, perturbation, clamp, vector smoothing: read before the call returned, the context owns FP64 copies)

    def push_slice_planar(self, t, planes, J=None, S=None, on_device=None):
        """ftkx_push_slice_planar / _f32: push_slice of the vector field whose components are `planes` (see _planes: nc = nd arrays or one
        (nc, ...) array, float32 or float64), interleaved -- and widened -- on the device.  J and S as in push_slice (interleaved).  Device
        planes are read before the call returns, never borrowed.  on_device as in push_scalar_slice"""
        ptrs, nc, keep, dev, f32 = _planes(planes)
        pj, kj, dj, fj = _ptr(J); ps, ks, ds, fs = _ptr(S)
        if any(p is not None and bool(d) != bool(dev) for p, d in ((pj, dj), (ps, ds))):
            raise ValueError("planes, J, S must all be host arrays or all device tensors")
        if any(p is not None and bool(f) != f32 for p, f in ((pj, fj), (ps, fs))):
            raise TypeError("the arrays of one push must all be float32 or all float64")
        if on_device is not None:
            if int(on_device) not in (0, 1, 2) or (int(on_device) != 0) != bool(dev):
                raise ValueError("on_device: 0 for host arrays, 1 or 2 for device tensors")
            dev = int(on_device)
        self._ck((self._L.ftkx_push_slice_planar_f32 if f32 else self._L.ftkx_push_slice_planar)(self._h, t, ptrs, nc, pj, ps, dev))
        owned = f32 or self._perturbing or self._clamping
        self._keep[t] = (kj, ks) if dev == 1 and not owned else None       # (J and S of FP64 on this device are borrowed; the planes never are)

    def temporal_push_planar(self, planes, on_device=None):
        """ftkx_temporal_push_planar / _f32: temporal_push(is_vector=True) of the vector snapshot whose components are `planes`"""
        ptrs, nc, keep, dev, f32 = _planes(planes)
        if on_device is not None:
            if int(on_device) not in (0, 1, 2) or (int(on_device) != 0) != bool(dev):
                raise ValueError("on_device: 0 for host arrays, 1 or 2 for device tensors")
            dev = int(on_device)
        t = C.c_int(-1)
        self._ck((self._L.ftkx_temporal_push_planar_f32 if f32 else self._L.ftkx_temporal_push_planar)(self._h, ptrs, nc, dev, C.byref(t)))
        if t.value >= 0:
            self._keep[t.value] = None
        return t.value

    def push_scalar_slice(self, t, S, on_device=None, keep_dtype=False):
        """on_device: None = 0 for a host array, 1 (borrowed) for a device tensor; 2: a device tensor, copied.
        keep_dtype=True: a float16 / bfloat16 / 8-, 16- or 32-bit integer array or tensor goes to the device with the element type it has
        (ftkx_push_scalar_slice_typed) and is widened there, exactly; it is read before the call returns and never borrowed.  float32 and
        float64 go where they go without it; any other element type raises TypeError"""
        ps, ks, ds, dt = _ptr_any(S, keep_dtype)
        f32 = dt == DTYPE_F32
        if on_device is not None:
            if int(on_device) not in (0, 1, 2) or (int(on_device) != 0) != bool(ds):
                raise ValueError("on_device: 0 for a host array, 1 or 2 for a device tensor")
            ds = int(on_device)
        if dt is not None and dt > DTYPE_F32:
            self._ck(self._L.ftkx_push_scalar_slice_typed(self._h, t, ps, dt, ds))
        else:
            self._ck((self._L.ftkx_push_scalar_slice_f32 if f32 else self._L.ftkx_push_scalar_slice)(self._h, t, ps, ds))
        owned = self._smoothing or self._perturbing or self._clamping or (dt is not None and dt != DTYPE_F64)
        self._keep[t] = ks if ds == 1 and not owned else None     # (2, smoothing, perturbation, clamp, float32: the context owns a copy)

    def drop_slice(self, t):
        self._ck(self._L.ftkx_drop_slice(self._h, t))
        self._keep.pop(t, None)
        for slot in (1, 2):
            self._let_go_aux(getattr(self, "_keep_aux", {}).pop((t, slot), None))

    def _let_go_aux(self, lent):
        """a lent aux tensor leaves its timestep: an armed series pass that is still open may read it (set_series_sampling) -- kept until the
        open passes have been completed"""
        if lent is not None and getattr(self, "_open_series", None):
            self._lent_under_passes = getattr(self, "_lent_under_passes", [])
            self._lent_under_passes.append(lent)

    # auxiliary scalar fields sampled at critical points (sample_kernels.hip)
    def push_aux_slice(self, t, slot, A, on_device=None):
        """ftkx_push_aux_slice / _f32: A -- one value per vertex of the array extent, float64 or float32 -- becomes the field that slot 1 or 2
        of the records is sampled from at timestep t.  on_device as for push_scalar_slice: None = 0 for a host array, 1 (lent: read where it
        lies) for a device tensor; 2: a device tensor, copied.  Smoothing, perturbation and clamp never apply"""
        pa, ka, da, f32 = _ptr(A)
        if on_device is not None:
            if int(on_device) not in (0, 1, 2) or (int(on_device) != 0) != bool(da):
                raise ValueError("on_device: 0 for a host array, 1 or 2 for a device tensor")
            da = int(on_device)
        n = getattr(self, "_n_vertices", None)
        if n is not None and ka is not None and int(ka.numel() if hasattr(ka, "numel") else ka.size) != n:
            raise FtkxError(_lib.E_INVALID, f"push_aux_slice: {int(ka.numel() if hasattr(ka, 'numel') else ka.size)} values for an array extent of {n} vertices")
        self._ck((self._L.ftkx_push_aux_slice_f32 if f32 else self._L.ftkx_push_aux_slice)(self._h, int(t), int(slot), pa, da))
        self._let_go_aux(self._keep_aux.get((int(t), int(slot))))      # (one that this push replaces)
        self._keep_aux[(int(t), int(slot))] = ka if da == 1 and not f32 else None      # (lent: alive until the slice is dropped)

    def sample_aux(self, records):
        """ftkx_sample_aux: scalar[1] / scalar[2] of every record, for the slots that have an aux array at all timesteps the records read, in
        place on a contiguous CP_DTYPE array (as a sweep returned it: the aux word says which element a record is); returns it"""
        if not (isinstance(records, np.ndarray) and records.dtype == CP_DTYPE and records.flags.c_contiguous and records.flags.writeable):
            raise TypeError("sample_aux: a contiguous, writeable CP_DTYPE array")
        self._ck(self._L.ftkx_sample_aux(self._h, records.ctypes.data, len(records)))
        return records

    def sample_counts(self):
        """(launches, records): launches of the sample kernel by sample_aux on this context so far, and the records they took"""
        a = C.c_ulonglong(0); b = C.c_ulonglong(0)
        self._ck(self._L.ftkx_debug_sample_counts(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def set_series_sampling(self, on=True):
        """ftkx_set_series_sampling: while on, sweep_series and sweep_series_submit / _complete return their records with scalar[1] /
        scalar[2] filled from the aux arrays, sampled on the device inside the pass (slots with an array at every slice the pass reads; a
        slot with arrays at some but not all: FtkxError -4 at submit).  Not while a pass is open (-1).  A lent aux tensor (on_device=1) that is
        dropped or replaced under open passes is kept referenced here until they have been completed"""
        self._ck(self._L.ftkx_set_series_sampling(self._h, 1 if on else 0))

    def series_sampled(self):
        """(slots, where) of the series pass completed last: the set of slots filled (bit 0: scalar[1], bit 1: scalar[2]); 0 not filled, 1 by
        the kernel inside the pass, 2 behind the host-driven batch inside the call"""
        s = C.c_uint(0); w = C.c_int(0)
        self._ck(self._L.ftkx_series_sampled(self._h, C.byref(s), C.byref(w)))
        return int(s.value), int(w.value)

    def series_sample_counts(self):
        """(launches, records, workgroups of the last launch) of the in-pass sample kernel on this context so far"""
        a = C.c_ulonglong(0); b = C.c_ulonglong(0); g = C.c_uint(0)
        self._ck(self._L.ftkx_debug_series_sample_counts(self._h, C.byref(a), C.byref(b), C.byref(g)))
        return int(a.value), int(b.value), int(g.value)

    def debug_sample_relaunch(self, records, reps):
        """profiling aid: the sample kernel over `records` `reps` times back to back -> device ms per launch (HIP events); nothing is written"""
        r = np.ascontiguousarray(records, dtype=CP_DTYPE)
        ms = (C.c_double * int(reps))()
        self._ck(self._L.ftkx_debug_sample_relaunch(self._h, r.ctypes.data, len(r), int(reps), ms))
        return list(ms)

    def slice_resolution(self, t):
        r, m = C.c_double(), C.c_double()
        self._ck(self._L.ftkx_slice_resolution(self._h, t, C.byref(r), C.byref(m)))
        return r.value, m.value

    def slices_resolution(self, ts):
        """slice_resolution for several resident slices with one launch and one synchronise -> {t: (resolution, max_abs)}"""
        ts = [int(t) for t in ts]
        n = len(ts)
        tt = (C.c_int * max(1, n))(*ts); r = (C.c_double * max(1, n))(); m = (C.c_double * max(1, n))()
        self._ck(self._L.ftkx_slices_resolution(self._h, tt, n, r, m))
        return {ts[i]: (r[i], m[i]) for i in range(n)}

    def slices_prepare(self, ts, factor_hint=0):
        """ftkx_slices_prepare: ONE pass over the slices builds the sweep's sign masks (under factor_hint, 0 = 256) and returns
        {t: (res_below, max_abs)} -- res_below = smallest non-zero |v| below 1 / factor_hint (DBL_MAX if none)"""
        ts = [int(t) for t in ts]
        n = len(ts)
        tt = (C.c_int * max(1, n))(*ts); r = (C.c_double * max(1, n))(); m = (C.c_double * max(1, n))()
        self._ck(self._L.ftkx_slices_prepare(self._h, tt, n, int(factor_hint), r, m))
        return {ts[i]: (r[i], m[i]) for i in range(n)}

    def sweep_announce(self, ts, scopes):
        """ftkx_sweep_announce: the sweeps that will be enqueued after the next slices_prepare, whose cull that call then queues
        right behind the mask kernel (a hint: collect uses the survivor list only if the pending sweeps are exactly these)"""
        n = len(ts)
        # (contiguous int32 numpy arrays are handed over as they are: a caller that announces the same sweeps every pass builds them once)
        if isinstance(ts, np.ndarray) and isinstance(scopes, np.ndarray) and ts.dtype == np.int32 and scopes.dtype == np.int32 and ts.flags.c_contiguous and scopes.flags.c_contiguous:
            self._ck(self._L.ftkx_sweep_announce(self._h, ts.ctypes.data, scopes.ctypes.data, n))
            return
        self._ck(self._L.ftkx_sweep_announce(self._h, (C.c_int * max(1, n))(*[int(t) for t in ts]), (C.c_int * max(1, n))(*[int(v) for v in scopes]), n))

    # ---- compact t-slab halo (torch tensors on this context's device, or on the host) ----
    def export_masks(self, t, torch, device):
        """owner side: (U uint8 tensor, word_index int32 tensor, words int64 tensor, mask_factor, max_abs) of a prepared slice"""
        ub, nw, mf, mx = C.c_size_t(), C.c_size_t(), C.c_ulonglong(), C.c_double()
        self._ck(self._L.ftkx_export_masks_size(self._h, int(t), C.byref(ub), C.byref(nw), C.byref(mf), C.byref(mx)))
        U = torch.empty((ub.value,), dtype=torch.uint8, device=device)
        idx = torch.empty((max(1, nw.value),), dtype=torch.int32, device=device)
        words = torch.empty((max(1, nw.value),), dtype=torch.int64, device=device)
        self._ck(self._L.ftkx_export_masks(self._h, int(t), U.data_ptr(), idx.data_ptr(), words.data_ptr(), 1 if U.is_cuda else 0))
        return U, idx[:nw.value], words[:nw.value], mf.value, mx.value

    def push_masked_slice(self, t, scalar_input, U, idx, words, mask_factor, max_abs):
        self._keep[("masked", t)] = (U, idx, words)
        self._ck(self._L.ftkx_push_masked_slice(self._h, int(t), int(bool(scalar_input)), U.data_ptr(), U.numel() * U.element_size(), idx.data_ptr() if len(idx) else None,
                                                words.data_ptr() if len(words) else None, len(idx), int(mask_factor), float(max_abs), 1 if U.is_cuda else 0))

    def packed_masks_bytes(self):
        """size of a packed mask message for this context's mesh (0: the mesh has no summarised masks), word capacity"""
        cap = C.c_size_t()
        n = self._L.ftkx_packed_masks_bytes(self._h, C.byref(cap))
        return int(n), int(cap.value)

    def export_masks_packed(self, t, out):
        """owner side: a prepared slice's masks as ONE message in `out` (uint8 tensor of packed_masks_bytes() bytes); a device tensor is
        filled by work queued on the context's stream -- nothing is waited for"""
        self._ck(self._L.ftkx_export_masks_packed(self._h, int(t), out.data_ptr(), 1 if out.is_cuda else 0))

    def push_masked_slice_packed(self, t, scalar_input, buf, mask_factor, max_abs):
        self._keep[("masked", t)] = buf
        self._ck(self._L.ftkx_push_masked_slice_packed(self._h, int(t), int(bool(scalar_input)), buf.data_ptr(), 1 if buf.is_cuda else 0, int(mask_factor), float(max_abs)))

    def sweep_cull(self, t_masked, torch, device):
        """receiver side, after sweep_enqueue: the cells (int64 tensor of core-linear indices) whose exact test reads the masked slice"""
        n = C.c_size_t()
        self._ck(self._L.ftkx_sweep_cull(self._h, int(t_masked), C.byref(n)))
        cells = torch.empty((max(1, n.value),), dtype=torch.int64, device=device)
        self._ck(self._L.ftkx_get_sparse_cells(self._h, cells.data_ptr(), 1 if cells.is_cuda else 0))
        return cells[:n.value]

    def sweep_enqueue_many(self, ts, scopes, factors):
        n = len(ts)
        if isinstance(ts, np.ndarray) and isinstance(scopes, np.ndarray) and ts.dtype == np.int32 and scopes.dtype == np.int32 and ts.flags.c_contiguous and scopes.flags.c_contiguous:
            f = np.ascontiguousarray(factors, dtype=np.uint64)     # (timesteps and scopes handed over as they are: built once by the caller)
            self._ck(self._L.ftkx_sweep_enqueue_many(self._h, ts.ctypes.data, scopes.ctypes.data, f.ctypes.data, n))
            return
        self._ck(self._L.ftkx_sweep_enqueue_many(self._h, (C.c_int * n)(*[int(t) for t in ts]), (C.c_int * n)(*[int(v) for v in scopes]),
                                                 (C.c_ulonglong * n)(*[int(f) for f in factors]), n))

    def sweep_series(self, ts, scopes, running_resolution=None, copy=True):
        """ftkx_sweep_series: the steps (ts[i], scopes[i]) over resident slices under the reference's sticky factor, formed on the
        device; one host wait.  -> (records, factors (uint64 array), running resolution after these slices).
        ts / scopes: int32 arrays (handed over as they are) or sequences."""
        n = len(ts)
        if not (isinstance(ts, np.ndarray) and ts.dtype == np.int32 and ts.flags.c_contiguous):
            ts = np.ascontiguousarray(ts, dtype=np.int32)
        if not (isinstance(scopes, np.ndarray) and scopes.dtype == np.int32 and scopes.flags.c_contiguous):
            scopes = np.ascontiguousarray(scopes, dtype=np.int32)
        run = C.c_double(np.finfo(np.float64).max if running_resolution is None else float(running_resolution))
        f = np.empty((max(1, n),), dtype=np.uint64)
        out, cnt = C.c_void_p(), C.c_size_t()
        self._ck(self._L.ftkx_sweep_series(self._h, ts.ctypes.data, scopes.ctypes.data, n, C.byref(run), f.ctypes.data, C.byref(out), C.byref(cnt)))
        return _lib.records_from(out.value, cnt.value, copy), f[:n], run.value

    def sweep_series_submit(self, ts, scopes, running_resolution=None, chain=False):
        """ftkx_sweep_series_submit: queue the pass and return.  chain=True: continue from the pass queued before it (still open)."""
        n = len(ts)
        ts = np.ascontiguousarray(ts, dtype=np.int32)
        scopes = np.ascontiguousarray(scopes, dtype=np.int32)
        if chain:
            run_p = None
        else:
            run = C.c_double(np.finfo(np.float64).max if running_resolution is None else float(running_resolution))
            run_p = C.addressof(run)
        self._ck(self._L.ftkx_sweep_series_submit(self._h, ts.ctypes.data, scopes.ctypes.data, n, run_p))
        self._open_series = getattr(self, "_open_series", [])
        self._open_series.append(n)

    def sweep_series_complete(self, copy=True):
        """ftkx_sweep_series_complete: the oldest open pass -> (records, factors, running resolution), as sweep_series returns them"""
        n = self._open_series.pop(0)
        run = C.c_double(0.0)
        f = np.empty((max(1, n),), dtype=np.uint64)
        out, cnt = C.c_void_p(), C.c_size_t()
        self._ck(self._L.ftkx_sweep_series_complete(self._h, C.byref(run), f.ctypes.data, C.byref(out), C.byref(cnt)))
        if not self._open_series:
            self._lent_under_passes = []      # (no pass is left that could read a lent aux tensor dropped meanwhile)
        return _lib.records_from(out.value, cnt.value, copy), f[:n], run.value

    # ---- the slab pass (ftkx_series_dist_*): one rank's device-driven pass, queued in stages; ftk_amd/tslab.py drives it ----
    def series_dist_cells(self):
        return int(self._L.ftkx_series_dist_cells(self._h))

    def series_dist_begin(self, ts, scopes, running_resolution, rank, nranks, upper, contrib, gathered, masks_out, side_stream=None):
        """upper: the rank that owns the slice behind this slab (None: no halo).  Tensors: device memory of this context's device
        (masks_out: None without a lower neighbour); side_stream: a hipStream_t (int) that is made to wait for masks_out only"""
        n = len(ts)
        ts = np.ascontiguousarray(ts, dtype=np.int32)
        scopes = np.ascontiguousarray(scopes, dtype=np.int32)
        run = C.c_double(np.finfo(np.float64).max if running_resolution is None else float(running_resolution))
        self._ck(self._L.ftkx_series_dist_begin(self._h, ts.ctypes.data, scopes.ctypes.data, n, C.byref(run), int(rank), int(nranks), -1 if upper is None else int(upper),
                                                contrib.data_ptr(), gathered.data_ptr(), masks_out.data_ptr() if masks_out is not None else None,
                                                C.c_void_p(side_stream) if side_stream else None))
        self._dist_n = n

    def series_dist_cull(self, masks_in, request_out):
        self._ck(self._L.ftkx_series_dist_cull(self._h, masks_in.data_ptr() if masks_in is not None else None, request_out.data_ptr() if request_out is not None else None))

    def series_dist_serve(self, request_in, reply_out):
        self._ck(self._L.ftkx_series_dist_serve(self._h, request_in.data_ptr() if request_in is not None else None, reply_out.data_ptr() if reply_out is not None else None))

    def series_dist_finish(self, reply_in):
        self._ck(self._L.ftkx_series_dist_finish(self._h, reply_in.data_ptr() if reply_in is not None else None))
        self._open_series = getattr(self, "_open_series", [])
        self._open_series.append(self._dist_n)

    def series_dist_status(self, nranks):
        """of the slab pass completed last -> (asked, served, gathered[nranks, 4])"""
        a, s_ = C.c_longlong(), C.c_longlong()
        g = np.zeros((nranks, 4), dtype=np.float64)
        self._ck(self._L.ftkx_series_dist_status(self._h, C.byref(a), C.byref(s_), g.ctypes.data, int(nranks)))
        return int(a.value), int(s_.value), g

    def sweep_series_abort(self):
        """ftkx_sweep_series_abort: discard the open passes (after a failed submit / complete, or to give up)"""
        self._open_series = []
        self._ck(self._L.ftkx_sweep_series_abort(self._h))
        self._lent_under_passes = []

    def series_last_path(self):
        """(path, status bits) of the last sweep_series: 1 device-driven (kernel chain), 2 finished by the fused tail, 4 one launch, 5 split (the
        chain next to the next pass's mask kernel), 0 host-driven batch"""
        st = C.c_ulonglong()
        return int(self._L.ftkx_series_last_path(self._h, C.byref(st))), int(st.value)

    def series_order(self):
        """ftkx_debug_series_order: {"nbins", "shift", "fullest", "rank_max"} of the ordering step of the series pass completed last (all
        zero where its records did not come through the bucket chain)"""
        o = (C.c_ulonglong * 4)()
        self._ck(self._L.ftkx_debug_series_order(self._h, o))
        return dict(nbins=int(o[0]), shift=int(o[1]), fullest=int(o[2]), rank_max=int(o[3]))

    def debug_sort_records(self, recs, key_bits):
        """ftkx_debug_sort_records: CP_DTYPE records through the host-driven batch's device sort (tags below 2 ** key_bits) -> a new array"""
        recs = np.ascontiguousarray(recs, dtype=CP_DTYPE)
        out = np.empty_like(recs)
        self._ck(self._L.ftkx_debug_sort_records(self._h, recs.ctypes.data, len(recs), int(key_bits), out.ctypes.data))
        return out

    def trace_last_path(self):
        """which way the last trace on this context went: 0 host, 1 device phases + host walks (ftkx_trace_curves_ctx), 2 all on the
        device (ftkx_trace_curves_device)"""
        return int(self._L.ftkx_trace_last_path(self._h))

    def post_process_last_path(self):
        """which way the last post-processing on this context went: 0 host, 2 all on the device (ftkx_post_process_curves_device,
        ftkx_pass2_device)"""
        return int(self._L.ftkx_post_process_last_path(self._h))

    def series_split_decision(self):
        """how this context decides on the split pass: {"state": "auto: measuring" | "auto: split" | "auto: in order" | "forced on" | "forced off",
        "median_in_order_ms", "median_split_ms"} (ftkx_series_split_decision)"""
        st, a, b = C.c_int(), C.c_double(), C.c_double()
        self._ck(self._L.ftkx_series_split_decision(self._h, C.byref(st), C.byref(a), C.byref(b)))
        names = ["auto: measuring", "auto: split", "auto: in order", "forced on", "forced off"]
        return {"state": names[st.value], "median_in_order_ms": a.value, "median_split_ms": b.value}

    def sweep_cancel(self):
        self._ck(self._L.ftkx_sweep_cancel(self._h))

    def patch_doubles(self):
        return int(self._L.ftkx_patch_doubles(self._h))

    def gather_patches(self, t, cells, torch):
        out = torch.empty((max(1, len(cells)) * self.patch_doubles(),), dtype=torch.float64, device=cells.device)
        if len(cells):
            self._ck(self._L.ftkx_gather_patches(self._h, int(t), cells.data_ptr(), len(cells), out.data_ptr(), 1 if cells.is_cuda else 0))
        return out[:len(cells) * self.patch_doubles()]

    def scatter_patches(self, t, cells, patches):
        if len(cells):
            self._ck(self._L.ftkx_scatter_patches(self._h, int(t), cells.data_ptr(), len(cells), patches.data_ptr(), 1 if cells.is_cuda else 0))

    def set_slice_resolution(self, t, resolution, max_abs):
        self._ck(self._L.ftkx_set_slice_resolution(self._h, t, float(resolution), float(max_abs)))

    def sweep(self, t, scope, factor):
        out, n = C.c_void_p(), C.c_size_t()
        self._ck(self._L.ftkx_sweep(self._h, t, scope, int(factor), C.byref(out), C.byref(n)))
        return _lib.records_from(out.value, n.value)

    def sweep_enqueue(self, t, scope, factor):
        self._ck(self._L.ftkx_sweep_enqueue(self._h, t, scope, int(factor)))

    def sweep_collect(self, copy=True):
        """copy=False: a view of the library's pinned host buffer, valid until the next sweep / collect on this context"""
        out, n = C.c_void_p(), C.c_size_t()
        self._ck(self._L.ftkx_sweep_collect(self._h, C.byref(out), C.byref(n)))
        return _lib.records_from(out.value, n.value, copy)

    def stats(self):
        s = Stats()
        self._ck(self._L.ftkx_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in Stats._fields_}

    KERNELS = ("mask_kernel", "cull_kernel", "exact_kernel", "tile_kernel")

    def invalidate_masks(self):
        self._ck(self._L.ftkx_invalidate_masks(self._h))

    def set_profiling(self, on=True):
        """0 / False off, 1 / True every kernel family, 2 the mask kernel only"""
        self._ck(self._L.ftkx_set_profiling(self._h, int(on)))

    def debug_tile_repeat(self, repeat):
        """profiling aid: the tile kernel's fan phase `repeat` times per tile and step from the next sweep on (1 = off)"""
        self._ck(self._L.ftkx_debug_tile_repeat(self._h, int(repeat)))

    def upload_counts(self):
        """(staged, direct): host arrays of this context that went up through the library's pinned staging / the runtime's own copy"""
        a = C.c_ulonglong(0); b = C.c_ulonglong(0)
        self._ck(self._L.ftkx_debug_upload_counts(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def kernel_times(self):
        """{kernel: (summed device ms, launches)} measured with HIP events on the context's stream"""
        ms = (C.c_double * 4)(); n = (C.c_ulonglong * 4)()
        self._ck(self._L.ftkx_get_kernel_times(self._h, ms, n))
        return {k: (ms[i], n[i]) for i, k in enumerate(self.KERNELS)}

    # derived fields on device tensors (ndarray/grad.hh)
    def gradient2D(self, S_ptr, DW, DH, V_ptr): self._ck(self._L.ftkx_gradient2D(self._h, S_ptr, DW, DH, V_ptr))
    def jacobian2D(self, V_ptr, DW, DH, symmetric, J_ptr): self._ck(self._L.ftkx_jacobian2D(self._h, V_ptr, DW, DH, int(symmetric), J_ptr))
    def gradient3D(self, S_ptr, DW, DH, DD, V_ptr): self._ck(self._L.ftkx_gradient3D(self._h, S_ptr, DW, DH, DD, V_ptr))
    def jacobian3D(self, V_ptr, DW, DH, DD, J_ptr): self._ck(self._L.ftkx_jacobian3D(self._h, V_ptr, DW, DH, DD, J_ptr))

    # spatial smoothing on device tensors (ndarray/conv.hh); weights: a host array of ksize ** nd doubles, x fastest
    def conv2D(self, S_ptr, DW, DH, weights, ksize, out_ptr, f32=False):
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.size != int(ksize) ** 2:
            raise ValueError("conv2D: ksize ** 2 weights")
        self._ck((self._L.ftkx_conv2D_f32 if f32 else self._L.ftkx_conv2D)(self._h, S_ptr, DW, DH, w.ctypes.data, int(ksize), out_ptr))

    def conv3D(self, S_ptr, DW, DH, DD, weights, ksize, out_ptr, f32=False):
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.size != int(ksize) ** 3:
            raise ValueError("conv3D: ksize ** 3 weights")
        self._ck((self._L.ftkx_conv3D_f32 if f32 else self._L.ftkx_conv3D)(self._h, S_ptr, DW, DH, DD, w.ctypes.data, int(ksize), out_ptr))

    # spatial smoothing of vector arrays on device pointers, every component as the scalar field it is (conv_vec_kernels.hip)
    def _conv_vec_weights(self, who, nd, weights, ksize):
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.size != int(ksize) ** nd:
            raise ValueError("%s: ksize ** %d weights" % (who, nd))
        return w

    def conv_vec(self, V_ptr, dims, weights, ksize, out_ptr, f32=False):
        """ftkx_conv2D_vec / ftkx_conv3D_vec (f32: a float32 source): out[c + nd * i] = conv(component c of V)[i], byte for byte what conv2D /
        conv3D give per component; dims: (DW, DH[, DD]); V and out: device addresses of nd * DW * DH (* DD) elements"""
        nd = len(dims)
        w = self._conv_vec_weights("conv_vec", nd, weights, ksize)
        d = [int(x) for x in dims]
        if nd == 2:
            self._ck((self._L.ftkx_conv2D_vec_f32 if f32 else self._L.ftkx_conv2D_vec)(self._h, V_ptr, d[0], d[1], w.ctypes.data, int(ksize), out_ptr))
        elif nd == 3:
            self._ck((self._L.ftkx_conv3D_vec_f32 if f32 else self._L.ftkx_conv3D_vec)(self._h, V_ptr, d[0], d[1], d[2], w.ctypes.data, int(ksize), out_ptr))
        else:
            raise ValueError("conv_vec: two or three extents")

    def conv_planar(self, plane_ptrs, dims, weights, ksize, out_ptr, f32=False):
        """ftkx_conv_planar / _f32: conv_vec of the vector array whose components are the nd planes at `plane_ptrs` (device addresses), smoothed
        and interleaved by the one kernel"""
        nd = len(dims)
        w = self._conv_vec_weights("conv_planar", nd, weights, ksize)
        if len(plane_ptrs) != nd:
            raise ValueError("conv_planar: one plane per dimension")
        d = [int(x) for x in dims] + [1] * (3 - nd)
        ptrs = (C.c_void_p * nd)(*[None if p is None else int(p) for p in plane_ptrs])
        self._ck((self._L.ftkx_conv_planar_f32 if f32 else self._L.ftkx_conv_planar)(self._h, nd, ptrs, d[0], d[1], d[2], w.ctypes.data, int(ksize), out_ptr))

    def conv_vec_counts(self):
        """(interleaved, planar, f32): launches of the vector smoothing's kernel by this context's pushes, by the source's form, and how many
        of them read float32"""
        a = C.c_ulonglong(0); b = C.c_ulonglong(0); c = C.c_ulonglong(0)
        self._ck(self._L.ftkx_debug_conv_vec_counts(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def debug_conv_vec_relaunch(self, src_ptrs, dims, weights, ksize, out_ptr, reps, planar=False, f32=False):
        """profiling aid: the vector smoothing's kernel `reps` times back to back -> device ms per launch (HIP events); src_ptrs: the nd
        planes (planar), else [V]"""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        d = [int(x) for x in dims] + [1] * (3 - len(dims))
        ptrs = (C.c_void_p * len(src_ptrs))(*[int(p) for p in src_ptrs])
        ms = (C.c_double * int(reps))()
        self._ck(self._L.ftkx_debug_conv_vec_relaunch(self._h, len(dims), ptrs, int(bool(planar)), int(bool(f32)), d[0], d[1], d[2], w.ctypes.data, int(ksize), out_ptr, int(reps), ms))
        return list(ms)

    # float32 -> FP64 on device pointers (widen_kernels.hip); conv2D / conv3D take f32=True for a float32 source
    def widen_f32(self, src_ptr, count, dst_ptr):
        """ftkx_widen_f32: dst[e] = double(src[e]) for `count` floats"""
        self._ck(self._L.ftkx_widen_f32(self._h, src_ptr, int(count), dst_ptr))

    def widen_typed(self, src_ptr, dtype, count, dst_ptr):
        """ftkx_widen_typed on device pointers: dst[e] = double(src[e]) for `count` elements of type `dtype` (DTYPE_F32 .. DTYPE_I32)"""
        self._ck(self._L.ftkx_widen_typed(self._h, src_ptr, int(dtype), int(count), dst_ptr))

    def debug_narrow_relaunch(self, src_ptr, dtype, count, dst_ptr, reps):
        """profiling aid: the narrow kernel `reps` times back to back -> device ms per launch (HIP events)"""
        ms = (C.c_double * int(reps))()
        self._ck(self._L.ftkx_debug_narrow_relaunch(self._h, src_ptr, int(dtype), int(count), dst_ptr, int(reps), ms))
        return list(ms)

    def narrow_counts(self):
        """launches of the narrow kernel by this context's pushes, a tuple indexed by DTYPE_* ([DTYPE_F64] and [DTYPE_F32] stay 0)"""
        n = (C.c_ulonglong * 10)()
        self._ck(self._L.ftkx_debug_narrow_counts(self._h, n))
        return tuple(int(v) for v in n)

    def debug_widen_relaunch(self, src_ptr, count, dst_ptr, reps):
        """profiling aid: the widen kernel `reps` times back to back -> device ms per launch (HIP events)"""
        ms = (C.c_double * int(reps))()
        self._ck(self._L.ftkx_debug_widen_relaunch(self._h, src_ptr, int(count), dst_ptr, int(reps), ms))
        return list(ms)

    # component planes -> interleaved FP64 on device pointers (concat_kernels.hip)
    def concat(self, plane_ptrs, count, dst_ptr, f32=False):
        """ftkx_concat / ftkx_concat_f32: dst[v * nc + k] = double(plane_k[v]) for `count` vertices; plane_ptrs: nc device addresses"""
        ptrs = (C.c_void_p * len(plane_ptrs))(*[None if p is None else int(p) for p in plane_ptrs])
        self._ck((self._L.ftkx_concat_f32 if f32 else self._L.ftkx_concat)(self._h, ptrs, len(plane_ptrs), int(count), dst_ptr))

    def debug_concat_relaunch(self, plane_ptrs, count, dst_ptr, reps, f32=False):
        """profiling aid: the concat kernel `reps` times back to back -> device ms per launch (HIP events)"""
        ptrs = (C.c_void_p * len(plane_ptrs))(*[int(p) for p in plane_ptrs])
        ms = (C.c_double * int(reps))()
        self._ck(self._L.ftkx_debug_concat_relaunch(self._h, ptrs, len(plane_ptrs), int(bool(f32)), int(count), dst_ptr, int(reps), ms))
        return list(ms)

    def planar_counts(self):
        """(vec, scalar): launches of the concat kernel by this context, with its 16-byte body / vertex by vertex"""
        a = C.c_ulonglong(0); b = C.c_ulonglong(0)
        self._ck(self._L.ftkx_debug_planar_counts(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def f32_counts(self):
        """(widened, convolved_direct): float32 arrays pushed into this context that took the widen kernel / went straight through the convolution"""
        a = C.c_ulonglong(0); b = C.c_ulonglong(0)
        self._ck(self._L.ftkx_debug_f32_counts(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def array_counts(self):
        """(allocated, pooled), each a tuple (field, mask, summary): slice arrays this context has had to allocate since it was made, and
        those that lie in its pool right now"""
        a = (C.c_ulonglong * 3)(); p = (C.c_ulonglong * 3)()
        self._ck(self._L.ftkx_debug_array_counts(self._h, a, p))
        return tuple(int(v) for v in a), tuple(int(v) for v in p)

    def debug_conv_relaunch(self, S_ptr, dims, weights, ksize, out_ptr, reps):
        """profiling aid: the convolution kernel `reps` times back to back -> device ms per launch (HIP events)"""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        d = [int(x) for x in dims] + [1] * (3 - len(dims))
        ms = (C.c_double * int(reps))()
        self._ck(self._L.ftkx_debug_conv_relaunch(self._h, len(dims), S_ptr, d[0], d[1], d[2], w.ctypes.data, int(ksize), out_ptr, int(reps), ms))
        return list(ms)


def _extract(nd, scope, current_timestep, domain, core, ext, Vc, Vn, Jc, Jn, Sc, Sn, factor, options, device_id, coords=None):
    L = _lib.load()
    keep = []
    ptrs = []
    for a in (Vc, Vn, Jc, Jn, Sc, Sn):
        if a is None:
            ptrs.append(None)
        else:
            a = np.ascontiguousarray(a, dtype=np.float64); keep.append(a); ptrs.append(a.ctypes.data)
    n4 = nd + 1
    lat = [_lib.ll(domain[0], n4), _lib.ll(domain[1], n4, 1), _lib.ll(core[0], n4), _lib.ll(core[1], n4, 1), _lib.ll(ext[0], 3), _lib.ll(ext[1], 3, 1)]
    out, n = C.c_void_p(), C.c_size_t()
    opt = C.byref(options) if options is not None else None
    if nd == 2:
        cc = None if coords is None else np.ascontiguousarray(coords, dtype=np.float64)
        rc = L.ftkx_extract_cp2dt(scope, current_timestep, *lat, *ptrs, 0 if cc is None else 1, None if cc is None else cc.ctypes.data, int(factor), opt, device_id,
                                  C.byref(out), C.byref(n))
    else:
        rc = L.ftkx_extract_cp3dt(scope, current_timestep, *lat, *ptrs, int(factor), opt, device_id, C.byref(out), C.byref(n))
    _lib.check(rc)
    recs = _lib.records_from(out.value, n.value)
    L.ftkx_free(out)
    return recs


def extract_cp2dt(scope, current_timestep, domain, core, ext, Vc, Vn, Jc, Jn, Sc, Sn, factor, options=None, device_id=0, coords=None):
    """extract_cp2dt_cuda's argument list (critical_point_tracker_2d_regular.hh:33-63); lattices as (starts, sizes) incl. time.
    coords: the boundary's explicit vertex coordinates, shape (DH, DW, 2) (use_explicit_coords = true), or None."""
    return _extract(2, scope, current_timestep, domain, core, ext, Vc, Vn, Jc, Jn, Sc, Sn, factor, options, device_id, coords)


def extract_cp3dt(scope, current_timestep, domain, core, ext, Vc, Vn, Jc, Jn, Sc, Sn, factor, options=None, device_id=0):
    """extract_cp3dt_cuda's argument list (critical_point_tracker_3d_regular.hh:42-56)."""
    return _extract(3, scope, current_timestep, domain, core, ext, Vc, Vn, Jc, Jn, Sc, Sn, factor, options, device_id)


def _trace_on_device(L, ctx, nd, domain, recs, out, tags=None):
    """ftkx_trace_curves_device on the records' tags, or on `tags`: a torch tensor (int64 / uint64 bit patterns) on the context's device"""
    if ctx is None:
        raise ValueError("device=True needs a Context: ftkx_trace_curves_device runs on its GPU")
    if tags is not None:
        if not tags.is_cuda or tags.dim() != 1 or not tags.is_contiguous() or tags.element_size() != 8:
            raise ValueError("tags: a contiguous 1-d tensor of 64-bit tags on the context's device")
        ptr, n, on_device = tags.data_ptr(), tags.numel(), 1
    else:
        host = np.ascontiguousarray(recs["tag"], dtype=np.uint64)
        ptr, n, on_device = host.ctypes.data, len(host), 0
    _lib.check(L.ftkx_trace_curves_device(ctx._h, nd, _lib.ll(domain[0]), _lib.ll(domain[1], fill=1), ptr, n, on_device, C.byref(out)), ctx._h)


def trace_curves(nd, domain, records, ctx=None, device=False, tags=None):
    """Pass 2 (ftkx_trace_curves): records (CP_DTYPE, element tags) -> (list of index arrays into `records`, loop flags, n_special).
    ctx: a Context whose GPU does the neighbour search and the component labelling (ftkx_trace_curves_ctx); same curves.
    device=True (needs ctx): seeds, walks and compaction on that GPU as well (ftkx_trace_curves_device); same curves.  With it,
    tags: the records' tags as a torch tensor already on the context's device (`records` may then be None)."""
    L = _lib.load()
    recs = None if records is None else np.ascontiguousarray(records, dtype=CP_DTYPE)
    out = _lib.Curves()
    if device:
        _trace_on_device(L, ctx, nd, domain, recs, out, tags)
    elif tags is not None:
        raise ValueError("tags: only with device=True")
    elif ctx is not None:
        _lib.check(L.ftkx_trace_curves_ctx(ctx._h, nd, _lib.ll(domain[0]), _lib.ll(domain[1], fill=1), recs.ctypes.data, len(recs), C.byref(out)), ctx._h)
    else:
        _lib.check(L.ftkx_trace_curves(nd, _lib.ll(domain[0]), _lib.ll(domain[1], fill=1), recs.ctypes.data, len(recs), C.byref(out)))
    offs = np.ctypeslib.as_array(out.offsets, shape=(out.n_curves + 1,)).copy()
    idx = np.ctypeslib.as_array(out.indices, shape=(max(1, out.n_points),))[:out.n_points].copy()
    loop = np.ctypeslib.as_array(out.loop, shape=(max(1, out.n_curves),))[:out.n_curves].copy()
    nspecial = out.n_special
    L.ftkx_free_curves(C.byref(out))
    return [idx[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)], loop, nspecial


class OnlineTracer:
    """ftkx_online_tracer: trace_critical_points_online (enable_streaming_trajectories) on record arrays"""

    def __init__(self, nd, domain):
        self._L = _lib.load()
        self._h = C.c_void_p()
        _lib.check(self._L.ftkx_online_tracer_create(C.byref(self._h), nd, _lib.ll(domain[0]), _lib.ll(domain[1], fill=1)))

    def grow(self, records):
        recs = np.ascontiguousarray(records, dtype=CP_DTYPE)
        _lib.check(self._L.ftkx_online_tracer_grow(self._h, recs.ctypes.data, len(recs)))

    def curves(self):
        """-> (list of record arrays, one per trajectory in order of birth; loop flags)"""
        pts, out = C.c_void_p(), _lib.Curves()
        _lib.check(self._L.ftkx_online_tracer_curves(self._h, C.byref(pts), C.byref(out)))
        n = out.n_points
        recs = np.frombuffer(C.string_at(pts.value, max(1, n) * CP_DTYPE.itemsize), dtype=CP_DTYPE)[:n].copy()
        offs = np.ctypeslib.as_array(out.offsets, shape=(out.n_curves + 1,)).copy()
        loop = np.ctypeslib.as_array(out.loop, shape=(max(1, out.n_curves),))[:out.n_curves].copy()
        self._L.ftkx_free(pts); self._L.ftkx_free_curves(C.byref(out))
        return [recs[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)], loop

    def close(self):
        if self._h:
            self._L.ftkx_online_tracer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TrajectorySet:
    """ftkx_trajectories as numpy arrays: curve c owns points offsets[c]:offsets[c+1]; per point the index into the record
    array, the (smoothed) type and the (adjusted) time; per curve the loop flag and its label in the reference's multimap."""

    def __init__(self, offsets, indices, type, t, loop, id):
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        self.indices = np.ascontiguousarray(indices, dtype=np.int64)
        self.type = np.ascontiguousarray(type, dtype=np.uint32)
        self.t = np.ascontiguousarray(t, dtype=np.float64)
        self.loop = np.ascontiguousarray(loop, dtype=np.int32)
        self.id = np.ascontiguousarray(id, dtype=np.int32)

    def __len__(self):
        return len(self.offsets) - 1

    def curve(self, c):
        a, b = self.offsets[c], self.offsets[c + 1]
        return self.indices[a:b], self.type[a:b], self.t[a:b], int(self.loop[c])

    @classmethod
    def _from_c(cls, out):
        n, npts = out.n_curves, out.n_points
        grab = lambda p, k: np.ctypeslib.as_array(p, shape=(max(1, k),))[:k].copy()  # noqa: E731
        return cls(np.ctypeslib.as_array(out.offsets, shape=(n + 1,)).copy(), grab(out.indices, npts), grab(out.type, npts), grab(out.t, npts),
                   grab(out.loop, n), grab(out.id, n))

    def _to_c(self):
        out = _lib.Trajectories()
        out.n_curves, out.n_points = len(self), len(self.indices)
        out.offsets = self.offsets.ctypes.data_as(C.POINTER(C.c_longlong)); out.indices = self.indices.ctypes.data_as(C.POINTER(C.c_longlong))
        out.loop = self.loop.ctypes.data_as(C.POINTER(C.c_int)); out.type = self.type.ctypes.data_as(C.POINTER(C.c_uint))
        out.t = self.t.ctypes.data_as(C.POINTER(C.c_double)); out.id = self.id.ctypes.data_as(C.POINTER(C.c_int))
        return out


def _curves_to_c(offsets, indices, loop):
    """(Curves, the arrays it points into) from numpy arrays"""
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    idx = np.ascontiguousarray(indices, dtype=np.int64)
    lp = np.ascontiguousarray(loop, dtype=np.int32)
    cur = _lib.Curves()
    cur.n_curves, cur.n_points, cur.n_special = len(lp), len(idx), 0
    cur.offsets = offs.ctypes.data_as(C.POINTER(C.c_longlong)); cur.indices = idx.ctypes.data_as(C.POINTER(C.c_longlong))
    cur.loop = lp.ctypes.data_as(C.POINTER(C.c_int))
    return cur, (offs, idx, lp)


def _post_process_c(L, recs, cur, ctx, device):
    if device and ctx is None:
        raise ValueError("device=True needs a Context: ftkx_post_process_curves_device runs on its GPU")
    out = _lib.Trajectories()
    if device:
        rc = L.ftkx_post_process_curves_device(ctx._h, recs.ctypes.data, len(recs), C.byref(cur), C.byref(out))
    else:
        rc = L.ftkx_post_process_curves(recs.ctypes.data, len(recs), C.byref(cur), C.byref(out))
    if rc != _lib.OK:
        L.ftkx_free_trajectories(C.byref(out))
    return rc, out


def post_process_curves(records, offsets, indices, loop, ctx=None, device=False):
    """ftkx_post_process_curves on curves given as arrays (curve c = indices[offsets[c]:offsets[c + 1]] into `records`, loop[c])
    -> TrajectorySet.  device=True (needs ctx): ftkx_post_process_curves_device on that context's GPU; same trajectories."""
    L = _lib.load()
    if device and ctx is None:
        raise ValueError("device=True needs a Context: ftkx_post_process_curves_device runs on its GPU")
    recs = np.ascontiguousarray(records, dtype=CP_DTYPE)
    cur, _keep = _curves_to_c(offsets, indices, loop)
    rc, out = _post_process_c(L, recs, cur, ctx, device)
    _lib.check(rc, ctx._h if device else None)
    ts = TrajectorySet._from_c(out)
    L.ftkx_free_trajectories(C.byref(out))
    return ts


def post_process(nd, domain, records, ctx=None, device=False):
    """ftkx_trace_curves followed by ftkx_post_process_curves (json_interface::post_process defaults) -> TrajectorySet.
    device=True (needs ctx): the post-processing on that context's GPU (ftkx_post_process_curves_device); same trajectories."""
    L = _lib.load()
    if device and ctx is None:
        raise ValueError("device=True needs a Context: ftkx_post_process_curves_device runs on its GPU")
    recs = np.ascontiguousarray(records, dtype=CP_DTYPE)
    cur = _lib.Curves()
    _lib.check(L.ftkx_trace_curves(nd, _lib.ll(domain[0]), _lib.ll(domain[1], fill=1), recs.ctypes.data, len(recs), C.byref(cur)))
    rc, out = _post_process_c(L, recs, cur, ctx, device)
    L.ftkx_free_curves(C.byref(cur))
    _lib.check(rc, ctx._h if device else None)
    ts = TrajectorySet._from_c(out)
    L.ftkx_free_trajectories(C.byref(out))
    return ts


def pass2(nd, domain, records, ctx=None, device=False, *, post_device=False):
    """ftkx_trace_curves (ctx given: ftkx_trace_curves_ctx, its data-parallel half on that context's GPU; device=True, which needs
    ctx: ftkx_trace_curves_device, all of it on that GPU), then ftkx_post_process_curves
    on its result, each timed by itself (the C calls only)
    -> (curves as index arrays, loop flags, n_special, TrajectorySet, ms_trace, ms_post_process)
    post_device=True (needs ctx): the post-processing on that GPU too.  With device=True it is ONE call, ftkx_pass2_device -- the curves
    stay on the device in between -- and ms_trace is the time of that call, ms_post_process 0; otherwise ftkx_post_process_curves_device
    on the curves the trace returned."""
    import time
    L = _lib.load()
    recs = np.ascontiguousarray(records, dtype=CP_DTYPE)
    cur = _lib.Curves()
    if device and ctx is None:
        raise ValueError("device=True needs a Context: ftkx_trace_curves_device runs on its GPU")
    if post_device and ctx is None:
        raise ValueError("post_device=True needs a Context: ftkx_post_process_curves_device runs on its GPU")
    tags = np.ascontiguousarray(recs["tag"], dtype=np.uint64) if device and not post_device else None
    out = _lib.Trajectories()
    t0 = time.perf_counter()
    if device and post_device:
        _lib.check(L.ftkx_pass2_device(ctx._h, nd, _lib.ll(domain[0]), _lib.ll(domain[1], fill=1), recs.ctypes.data, len(recs), C.byref(cur), C.byref(out)), ctx._h)
        rc = _lib.OK
        t1 = t2 = time.perf_counter()
    else:
        if device:
            _lib.check(L.ftkx_trace_curves_device(ctx._h, nd, _lib.ll(domain[0]), _lib.ll(domain[1], fill=1), tags.ctypes.data, len(tags), 0, C.byref(cur)), ctx._h)
        elif ctx is not None:
            _lib.check(L.ftkx_trace_curves_ctx(ctx._h, nd, _lib.ll(domain[0]), _lib.ll(domain[1], fill=1), recs.ctypes.data, len(recs), C.byref(cur)), ctx._h)
        else:
            _lib.check(L.ftkx_trace_curves(nd, _lib.ll(domain[0]), _lib.ll(domain[1], fill=1), recs.ctypes.data, len(recs), C.byref(cur)))
        t1 = time.perf_counter()
        rc, out = _post_process_c(L, recs, cur, ctx, post_device)
        t2 = time.perf_counter()
    offs = np.ctypeslib.as_array(cur.offsets, shape=(cur.n_curves + 1,)).copy()
    idx = np.ctypeslib.as_array(cur.indices, shape=(max(1, cur.n_points),))[:cur.n_points].copy()
    loop = np.ctypeslib.as_array(cur.loop, shape=(max(1, cur.n_curves),))[:cur.n_curves].copy()
    nspecial = cur.n_special
    L.ftkx_free_curves(C.byref(cur))
    _lib.check(rc, ctx._h if post_device else None)
    ts = TrajectorySet._from_c(out)
    L.ftkx_free_trajectories(C.byref(out))
    return [idx[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)], loop, nspecial, ts, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def trace_and_post_process(nd, domain, records):
    """post_process() as a list of (indices, types, t, loop) per trajectory."""
    ts = post_process(nd, domain, records)
    return [ts.curve(c) for c in range(len(ts))]


def _format(path, format):
    if format is None:
        return _lib.load().ftkx_format_from_path(str(path).encode())
    return {"binary": FORMAT_BINARY, "json": FORMAT_JSON, "text": FORMAT_TEXT}.get(format, format)


def _names(scalar_names):
    if scalar_names is None:
        return None, -1
    arr = (C.c_char_p * max(1, len(scalar_names)))(*[s.encode() for s in scalar_names])
    return arr, len(scalar_names)


def write_critical_points(path, records, format=None, v=None, id=None, scalar_names=None):
    """critical_point_tracker::write_critical_points_{json,binary,text}; format None = by file name (txt / json / else binary)."""
    recs = np.ascontiguousarray(records, dtype=CP_DTYPE)
    vv = None if v is None else np.ascontiguousarray(v, dtype=np.float64).reshape(len(recs), 3)
    ii = None if id is None else np.ascontiguousarray(id, dtype=np.uint64)
    names, nn = _names(scalar_names)
    _lib.check(_lib.load().ftkx_write_critical_points(str(path).encode(), _format(path, format), recs.ctypes.data, len(recs),
                                                      None if vv is None else vv.ctypes.data, None if ii is None else ii.ctypes.data, names, nn))


def read_critical_points(path, format=None):
    """read_critical_points_{json,binary} -> (records[CP_DTYPE] with the aux word, v[n,3], id[n])"""
    L = _lib.load()
    r, v, i, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
    _lib.check(L.ftkx_read_critical_points(str(path).encode(), _format(path, format), C.byref(r), C.byref(n), C.byref(v), C.byref(i)))
    k = n.value
    recs = np.frombuffer(C.string_at(r.value, k * CP_DTYPE.itemsize), dtype=CP_DTYPE).copy()
    vv = np.frombuffer(C.string_at(v.value, k * 24), dtype=np.float64).reshape(k, 3).copy()
    ii = np.frombuffer(C.string_at(i.value, k * 8), dtype=np.uint64).copy()
    for p in (r, v, i):
        L.ftkx_free(p)
    return recs, vv, ii


def write_traced_critical_points(path, records, trajectories, format=None, scalar_names=None):
    """write_traced_critical_points_{json,binary,text} of a TrajectorySet over `records`."""
    recs = np.ascontiguousarray(records, dtype=CP_DTYPE)
    tr = trajectories._to_c()
    names, nn = _names(scalar_names)
    _lib.check(_lib.load().ftkx_write_traced_critical_points(str(path).encode(), _format(path, format), recs.ctypes.data, len(recs), C.byref(tr), names, nn))


def read_traced_critical_points(path, format=None):
    """read_traced_critical_points_{json,binary} -> (records in file order, TrajectorySet indexing them)"""
    L = _lib.load()
    r, n, out = C.c_void_p(), C.c_size_t(), _lib.Trajectories()
    _lib.check(L.ftkx_read_traced_critical_points(str(path).encode(), _format(path, format), C.byref(r), C.byref(n), C.byref(out)))
    recs = np.frombuffer(C.string_at(r.value, n.value * CP_DTYPE.itemsize), dtype=CP_DTYPE).copy()
    ts = TrajectorySet._from_c(out)
    L.ftkx_free(r); L.ftkx_free_trajectories(C.byref(out))
    return recs, ts


class _TrackerRegular:
    """ftkx::critical_point_tracker_regular (include/ftkx_tracker.hh) through its C handle; method names are the reference's."""
    ND = 0

    def __init__(self, device_id=0, device_ids=None, block=2):
        """device_ids: several GPUs behind one tracker (timesteps dealt to them in blocks of `block` steps, one host thread per
        device; a device may be listed more than once)"""
        self._L = _lib.load()
        self._h = C.c_void_p()
        if device_ids is not None:
            ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
            _lib.check(self._L.ftkx_tracker_create_multi(C.byref(self._h), self.ND, ids, len(device_ids), int(block)), None, True)
        else:
            _lib.check(self._L.ftkx_tracker_create(C.byref(self._h), self.ND, device_id), None, True)
        self._src = [SOURCE_NONE, SOURCE_NONE, SOURCE_NONE, 0]
        self._flags = dict(robust=1, use_type_filter=0, type_filter=0, compute_degrees=0, exact_only=0, tag_mode=TAG_REFERENCE)
        self._keep = []

    def close(self):
        if self._h:
            self._L.ftkx_tracker_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        _lib.check(rc, self._h, True)

    def set_domain(self, starts, sizes): self._ck(self._L.ftkx_tracker_set_domain(self._h, _lib.ll(starts), _lib.ll(sizes, fill=1)))
    def set_array_domain(self, starts, sizes): self._ck(self._L.ftkx_tracker_set_array_domain(self._h, _lib.ll(starts), _lib.ll(sizes, fill=1)))
    def set_scalar_field_source(self, s): self._src[0] = s
    def set_vector_field_source(self, s): self._src[1] = s
    def set_jacobian_field_source(self, s): self._src[2] = s
    def set_jacobian_symmetric(self, b): self._src[3] = int(b)
    def set_enable_robust_detection(self, b): self._flags["robust"] = int(b)
    def set_enable_computing_degrees(self, b): self._flags["compute_degrees"] = int(b)
    def set_type_filter(self, f): self._flags["use_type_filter"] = 1; self._flags["type_filter"] = int(f)
    def set_exact_only(self, b): self._flags["exact_only"] = int(b)
    def set_tag_mode(self, m): self._flags["tag_mode"] = int(m)
    def set_stream(self, ptr): self._ck(self._L.ftkx_tracker_set_stream(self._h, C.c_void_p(ptr)))
    def set_current_timestep(self, t): self._ck(self._L.ftkx_tracker_set_current_timestep(self._h, int(t)))
    def set_deferred_collection(self, b, depth=1):
        """the sweep of step t + 1 is queued before the records of step t are collected (ftkx_tracker.hh); depth > 1: the sweeps of `depth`
        consecutive steps are queued as one pass.  Pushed device tensors are kept alive until their batch has been collected"""
        self._deferred = bool(b)
        self._deferred_depth = max(1, int(depth)) if b else 1
        self._ck(self._L.ftkx_tracker_set_deferred_collection(self._h, self._deferred_depth if b else 0))

    def set_trace_on_device(self, b):
        """finalize() traces the curves entirely on the tracker's GPU (ftkx_trace_curves_device); same curves; off by default"""
        self._ck(self._L.ftkx_tracker_set_trace_on_device(self._h, int(bool(b))))

    def set_spatial_smoothing(self, sigma, ksize=3):
        """before initialize(): every scalar snapshot is smoothed on the device like the reference stream's --spatial-smoothing-kernel
        (conv_gaussian(snapshot, sigma, ksize, ksize // 2)); ksize 0: off"""
        self._ck(self._L.ftkx_tracker_set_spatial_smoothing(self._h, float(sigma), int(ksize)))

    def set_vector_spatial_smoothing(self, sigma, ksize=3):
        """before initialize(): every vector snapshot (push_vector_field_snapshot, push_vector_field_components) has each component
        smoothed on the device as the scalar field it is (conv_gaussian(component, sigma, ksize, ksize // 2), one kernel); ksize 0: off"""
        self._ck(self._L.ftkx_tracker_set_vector_spatial_smoothing(self._h, float(sigma), int(ksize)))

    def set_perturbation(self, sigma, seed=0):
        """before initialize(): every snapshot gets sigma * N(0, 1) noise on the device like the reference stream's "perturbation", the noise
        of element e of timestep t being a function of (seed, t, e) alone; sigma 0: off"""
        self._ck(self._L.ftkx_tracker_set_perturbation(self._h, float(sigma), int(seed)))

    def set_clamp(self, lo=None, hi=None):
        """before initialize(): every snapshot becomes min(max(lo, x), hi) on the device like the reference stream's "clamp"; no bounds: off"""
        on = lo is not None or hi is not None
        if on and (lo is None or hi is None):
            raise ValueError("set_clamp: both bounds, or none")
        self._ck(self._L.ftkx_tracker_set_clamp(self._h, int(on), float(lo) if on else 0.0, float(hi) if on else 0.0))

    def set_sampling_in_pass(self, b=True):
        """before initialize(): with components named (set_scalar_components), every step's device-driven pass fills scalar[1] / scalar[2]
        itself (Context.set_series_sampling) instead of a pass over the finished records -- which allows deferred collection, single steps
        and batches, with components.  Same points and curves, bit for bit.  Default off"""
        self._ck(self._L.ftkx_tracker_set_sampling_in_pass(self._h, int(bool(b))))

    def set_temporal_smoothing(self, sigma, ksize=5):
        """before initialize(): the pushed snapshots are raw and feed the reference stream's temporal filter on the device; the tracker sees
        the smoothed series, ksize // 2 pushes late (snapshots_from_last_push, flush_temporal_smoothing); ksize 0: off"""
        self._ck(self._L.ftkx_tracker_set_temporal_smoothing(self._h, float(sigma), int(ksize)))

    def snapshots_from_last_push(self):
        """0 or 1: whether the last push_* appended a snapshot (always 1 without temporal smoothing)"""
        n = C.c_int(0)
        self._ck(self._L.ftkx_tracker_snapshots_from_last_push(self._h, C.byref(n)))
        return n.value

    def flush_temporal_smoothing(self):
        """after the last push: appends one trailing smoothed snapshot -> True, or False when none is left; loop it in front of finalize(),
        with advance_timestep() between the calls"""
        n = C.c_int(0)
        self._ck(self._L.ftkx_tracker_flush_temporal_smoothing(self._h, C.byref(n)))
        return bool(n.value)

    def trace_last_path(self):
        """Context.trace_last_path() of the tracker's (first) context"""
        return int(self._L.ftkx_tracker_trace_last_path(self._h))

    def set_post_process_on_device(self, b):
        """with set_trace_on_device(True): post_process() on the tracker's GPU as well (ftkx_post_process_curves_device); same trajectories"""
        self._ck(self._L.ftkx_tracker_set_post_process_on_device(self._h, int(bool(b))))

    def post_process_last_path(self):
        """Context.post_process_last_path() of the tracker's (first) context"""
        return int(self._L.ftkx_tracker_post_process_last_path(self._h))

    # several ranks behind the tracker (include/ftkx_tracker.hh: slab mode): this rank's tracker takes the snapshots of its timestep slab
    # (tslab.slab_range), sweeps it as one device-driven pass, finalize() gathers the points on rank 0.  Pushed device tensors are kept alive.
    def set_communicator(self, nccl_comm, rank, nranks, nt):
        self._slab_keep = []
        self._ck(self._L.ftkx_tracker_set_communicator(self._h, nccl_comm, int(rank), int(nranks), int(nt)))

    def set_slab_hub(self, hub, rank, nt):
        self._slab_keep = []
        self._ck(self._L.ftkx_tracker_set_slab_hub(self._h, hub, int(rank), int(nt)))

    def set_enable_streaming_trajectories(self, b): self._ck(self._L.ftkx_tracker_set_enable_streaming_trajectories(self._h, int(bool(b))))
    def set_coords_bounds(self, b): self._ck(self._L.ftkx_tracker_set_coords_bounds(self._h, (C.c_double * len(b))(*[float(x) for x in b])))

    def set_coords_rectilinear(self, arrays):
        """REGULAR_COORDS_RECTILINEAR: one 1-D float64 array per axis, indexed by the vertex coordinate"""
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays] + [None] * (3 - len(arrays))
        args = []
        for a in arrs:
            args += [a.ctypes.data if a is not None else None, len(a) if a is not None else 0]
        self._ck(self._L.ftkx_tracker_set_coords_rectilinear(self._h, *args))

    def set_coords_explicit(self, coords):
        """REGULAR_COORDS_EXPLICIT: numpy array of shape (n1, n0, ncomp) = the reference's ndarray (ncomp, n0, n1)"""
        e = np.ascontiguousarray(coords, dtype=np.float64)
        self._ck(self._L.ftkx_tracker_set_coords_explicit(self._h, e.ctypes.data, e.shape[-1], e.shape[-2], e.shape[-3]))

    def initialize(self):
        self._ck(self._L.ftkx_tracker_set_sources(self._h, *self._src))
        f = self._flags
        self._ck(self._L.ftkx_tracker_set_flags(self._h, f["robust"], f["use_type_filter"], f["type_filter"], f["compute_degrees"], f["exact_only"], f["tag_mode"]))
        self._ck(self._L.ftkx_tracker_initialize(self._h))

    def set_scalar_components(self, names):
        """critical_point_tracker::set_scalar_components: one to three names; the first names scalar[0] (the tracker's own scalar field), the
        others the extra fields every push then brings as components=[...], sampled at the critical points into scalar[1] and scalar[2]"""
        names = [str(n).encode() for n in names]
        self._ck(self._L.ftkx_tracker_set_scalar_components(self._h, (C.c_char_p * max(1, len(names)))(*names), len(names)))

    def _push_extra(self, kind, s, v, j, components):
        """a push_* call with the snapshot's extra scalar fields (all arrays of one call: one dtype, one place)"""
        got = [_ptr(a) for a in (s, v, j)] + [_ptr(a) for a in components]
        given = [g for g in got if g[0] is not None]
        f32 = _same_type(*[g[3] for g in given])
        if len({g[2] for g in given}) > 1:
            raise ValueError("the arrays of one push must all be host arrays or all device tensors")
        dev = given[0][2] if given else 0
        extra = (C.c_void_p * max(1, len(components)))(*[g[0] for g in got[3:]])
        self._keep.append(None if f32 else tuple(g[1] for g in got))
        self._ck(self._L.ftkx_tracker_push_snapshot_extra(self._h, kind, got[0][0], got[1][0], got[2][0], extra, len(components), dev, int(f32)))

    def _narrow(self, keep_dtype, components, *arrays):
        """keep_dtype=True: the one element type of the arrays of a push where it is narrower than float32 (they then go to the typed
        entries as they are: (addresses, on_device, DTYPE_*, keepalives)), else None: the push goes the way it goes without keep_dtype.
        The keepalives are the arrays the addresses point into -- the contiguous copies of views that were not contiguous among them --
        and the caller holds the tuple until the library has read them (it reads before it returns).  Raises TypeError for an element
        type the library does not take; narrow snapshots come without extra components"""
        if not keep_dtype:
            return None
        got = [_ptr_typed(a) for a in arrays] + [_ptr_typed(a) for a in (components or [])]
        dt = _one_dtype(*[g[3] for g in got])
        if dt <= DTYPE_F32:
            return None
        if components is not None:
            raise TypeError("keep_dtype: extra scalar components are float32 or float64")
        if len({g[2] for g in got if g[0] is not None}) > 1:
            raise ValueError("the arrays of one push must all be host arrays or all device tensors")
        self._keep.append(None)                                            # (read before the call returns, never borrowed)
        return [g[0] for g in got], next(g[2] for g in got if g[0] is not None), dt, [g[1] for g in got]

    def push_scalar_field_snapshot(self, s, components=None, keep_dtype=False):
        """keep_dtype=True: a float16 / bfloat16 / 8-, 16- or 32-bit integer snapshot goes to the device with the element type it has and is
        widened there (Context.push_scalar_slice); any element type the library does not take raises TypeError"""
        narrow = self._narrow(keep_dtype, components, s)
        if narrow:
            rc = self._L.ftkx_tracker_push_scalar_field_snapshot_typed(self._h, narrow[0][0], narrow[2], narrow[1])      # (`narrow` holds the arrays until here)
            return self._ck(rc)
        if components is not None:
            return self._push_extra(0, s, None, None, list(components))
        p, k, d, f32 = _ptr(s); self._keep.append(None if f32 else k)      # (float32: read before the call returns, never borrowed)
        self._ck((self._L.ftkx_tracker_push_scalar_field_snapshot_f32 if f32 else self._L.ftkx_tracker_push_scalar_field_snapshot)(self._h, p, d))

    def push_vector_field_snapshot(self, v, components=None, keep_dtype=False):
        narrow = self._narrow(keep_dtype, components, v)
        if narrow:
            rc = self._L.ftkx_tracker_push_vector_field_snapshot_typed(self._h, narrow[0][0], narrow[2], narrow[1])
            return self._ck(rc)
        if components is not None:
            return self._push_extra(1, None, v, None, list(components))
        p, k, d, f32 = _ptr(v); self._keep.append(None if f32 else k)
        self._ck((self._L.ftkx_tracker_push_vector_field_snapshot_f32 if f32 else self._L.ftkx_tracker_push_vector_field_snapshot)(self._h, p, d))

    def push_vector_field_components(self, planes):
        """push_vector_field_snapshot of the vector field whose components are `planes` (nc arrays, or one (nc, ...) array; float32 or
        float64; host or device), interleaved on the device.  Read before the call returns, never borrowed"""
        ptrs, nc, keep, dev, f32 = _planes(planes); self._keep.append(None)
        self._ck((self._L.ftkx_tracker_push_vector_field_components_f32 if f32 else self._L.ftkx_tracker_push_vector_field_components)(self._h, ptrs, nc, dev))

    def push_field_data_snapshot(self, s, v, j, components=None, keep_dtype=False):
        narrow = self._narrow(keep_dtype, components, s, v, j)
        if narrow:
            rc = self._L.ftkx_tracker_push_field_data_snapshot_typed(self._h, narrow[0][0], narrow[0][1], narrow[0][2], narrow[2], narrow[1])
            return self._ck(rc)
        if components is not None:
            return self._push_extra(2, s, v, j, list(components))
        ps, ks, ds, fs = _ptr(s); pv, kv, dv, fv = _ptr(v); pj, kj, dj, fj = _ptr(j)
        f32 = _same_type(*[f for p, f in ((ps, fs), (pv, fv), (pj, fj)) if p is not None])
        self._keep.append(None if f32 else (ks, kv, kj))
        self._ck((self._L.ftkx_tracker_push_field_data_snapshot_f32 if f32 else self._L.ftkx_tracker_push_field_data_snapshot)(self._h, ps, pv, pj, dv))

    def advance_timestep(self):
        self._ck(self._L.ftkx_tracker_advance_timestep(self._h))
        if hasattr(self, "_slab_keep"):             # slab mode: the snapshots stay resident until the slab's pass has run
            self._slab_keep += self._keep
        self._keep = self._keep[-((3 * getattr(self, "_deferred_depth", 1) + 2) if getattr(self, "_deferred", False) else 2):]

    def update_timestep(self): self._ck(self._L.ftkx_tracker_update_timestep(self._h))

    def reset(self):
        """critical_point_tracker_regular::reset: the points and the queued snapshots go, the next push is timestep 0; a temporal filter is emptied"""
        self._ck(self._L.ftkx_tracker_reset(self._h))
        self._keep = []

    def sync(self): self._ck(self._L.ftkx_tracker_sync(self._h))

    def get_critical_points(self):
        """(records[CP_DTYPE], ordinal[int32], timestep[int32]) in the reference's std::map order (by element tag)"""
        n = C.c_size_t()
        self._ck(self._L.ftkx_tracker_num_critical_points(self._h, C.byref(n)))
        recs = np.zeros(n.value, dtype=CP_DTYPE); o = np.zeros(n.value, dtype=np.int32); ts = np.zeros(n.value, dtype=np.int32)
        if n.value:
            self._ck(self._L.ftkx_tracker_get_critical_points(self._h, recs.ctypes.data, o.ctypes.data, ts.ctypes.data, n.value))
        return recs, o, ts

    def finalize(self): self._ck(self._L.ftkx_tracker_finalize(self._h))

    def get_traced_critical_points(self):
        """after finalize(): (list of tag arrays, one per curve, in curve order; loop flags)"""
        nc, npts = C.c_size_t(), C.c_size_t()
        self._ck(self._L.ftkx_tracker_num_curves(self._h, C.byref(nc), C.byref(npts)))
        offs = np.zeros(nc.value + 1, dtype=np.int64); tags = np.zeros(max(1, npts.value), dtype=np.uint64); loop = np.zeros(max(1, nc.value), dtype=np.int32)
        self._ck(self._L.ftkx_tracker_get_curves(self._h, offs.ctypes.data, tags.ctypes.data, loop.ctypes.data))
        return [tags[offs[i]:offs[i + 1]] for i in range(nc.value)], loop[:nc.value]

    def get_traced_scalars(self):
        """after finalize(): per curve an array (points, 3) of scalar[0 .. 2], in the order of get_traced_critical_points()"""
        curves, _ = self.get_traced_critical_points()
        npts = sum(len(c) for c in curves)
        sc = np.zeros((max(1, npts), 3), dtype=np.float64)
        self._ck(self._L.ftkx_tracker_get_curve_scalars(self._h, sc.ctypes.data))
        out, k = [], 0
        for c in curves:
            out.append(sc[k:k + len(c)]); k += len(c)
        return out

    def post_process(self):
        """json_interface::post_process with its default options, on the traced curves"""
        self._ck(self._L.ftkx_tracker_post_process(self._h))

    def get_traced_trajectories(self):
        """after finalize() [+ post_process()]: list of (tags, types, t, loop, label) per curve"""
        curves, loop = self.get_traced_critical_points()
        npts = sum(len(c) for c in curves)
        ty = np.zeros(max(1, npts), dtype=np.uint32); tt = np.zeros(max(1, npts), dtype=np.float64); ids = np.zeros(max(1, len(curves)), dtype=np.int32)
        self._ck(self._L.ftkx_tracker_get_curve_points(self._h, ty.ctypes.data, tt.ctypes.data, ids.ctypes.data))
        out, k = [], 0
        for i, c in enumerate(curves):
            out.append((c, ty[k:k + len(c)], tt[k:k + len(c)], int(loop[i]), int(ids[i]))); k += len(c)
        return out

    def _write(self, path, fmt, traced): self._ck(self._L.ftkx_tracker_write(self._h, str(path).encode(), fmt, traced))
    def write_critical_points_json(self, path): self._write(path, FORMAT_JSON, 0)
    def write_critical_points_binary(self, path): self._write(path, FORMAT_BINARY, 0)
    def write_critical_points_text(self, path): self._write(path, FORMAT_TEXT, 0)
    def write_traced_critical_points_json(self, path): self._write(path, FORMAT_JSON, 1)
    def write_traced_critical_points_binary(self, path): self._write(path, FORMAT_BINARY, 1)
    def write_traced_critical_points_text(self, path): self._write(path, FORMAT_TEXT, 1)
    def read_critical_points_json(self, path): self._ck(self._L.ftkx_tracker_read_critical_points(self._h, str(path).encode(), FORMAT_JSON))
    def read_critical_points_binary(self, path): self._ck(self._L.ftkx_tracker_read_critical_points(self._h, str(path).encode(), FORMAT_BINARY))

    def get_vector_field_scaling_factor(self):
        f, r = C.c_ulonglong(), C.c_double()
        self._ck(self._L.ftkx_tracker_get_scaling(self._h, C.byref(f), C.byref(r)))
        return f.value

    def get_last_stats(self):
        s = Stats()
        self._ck(self._L.ftkx_tracker_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in Stats._fields_}


class CriticalPointTracker2DRegular(_TrackerRegular):
    ND = 2


class CriticalPointTracker3DRegular(_TrackerRegular):
    ND = 3
