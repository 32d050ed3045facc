"""Torch-facing wrappers over the C ABI (device tensors in, device tensors out, current stream).

Every function here launches HIP kernels from libmepol_amd.so; none has a CPU path.  Tensors
must live on a ROCm device; dtypes follow the reference (f64 values, int64 indices at the
API boundary; int32 indices internally).
"""
import ctypes
import math
import threading

import torch

from . import _lib
from ._lib import call, ptr

_WS = {}


def _stream():
    return ctypes_void(torch.cuda.current_stream().cuda_stream)


def ctypes_void(v):
    return ctypes.c_void_p(v)


def _require_device(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("mepol_amd ops need ROCm device tensors (got a CPU tensor); "
                             "there is no CPU path in the product")


def _workspace(device, nbytes, tag="knn"):
    """Scratch for eager calls, one buffer per (tag, device, stream): calls on one stream are
    ordered, so they may share it; a buffer outgrown on a stream is released through the caching
    allocator, which is stream-aware.  Captured graphs (algorithms/device_loop.py) never use this
    cache: they own their scratch (see head_workspace / layer_workspace)."""
    key = (tag, device, torch.cuda.current_stream(device).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def _ws_bytes(op, *sizes):
    """Bytes of scratch mepol_<op> needs at these sizes (its mepol_<op>_workspace_size)."""
    nbytes = ctypes.c_size_t()
    call(f"mepol_{op}_workspace_size", *sizes, ctypes.byref(nbytes))
    return nbytes.value


def _own_workspace(device, op, *sizes):
    return torch.empty(max(_ws_bytes(op, *sizes), 1), dtype=torch.uint8, device=device)


def _ws_or_cached(ws, device, tag, op, *sizes):
    """The caller's `ws`, or the per-stream eager buffer `tag` grown to what mepol_<op> needs."""
    return ws if ws is not None else _workspace(device, _ws_bytes(op, *sizes), tag=tag)


def head_workspace(n, hidden, a, device):
    """A caller-owned scratch buffer for head_backward at these sizes."""
    return _own_workspace(device, "head", n, hidden, a)


def layer_workspace(n, f, out, device):
    """A caller-owned scratch buffer for layer_backward at these sizes."""
    return _own_workspace(device, "layer", n, f, out)


def dh1_layer1_workspace(n, h0, f, device):
    """A caller-owned scratch buffer for dh1_layer1_backward at these sizes."""
    return _own_workspace(device, "dh1_layer1", n, h0, f)


def knn_plan(n_cand, n_query, d, kp1, split=0):
    ks, lst, sp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    call("mepol_knn_plan_info", n_cand, n_query, d, kp1, split, ctypes.byref(ks),
         ctypes.byref(lst), ctypes.byref(sp))
    # ks == 0: no f16 screen (d > 63 or k+1 > 60): every query takes the exhaustive f64 scan,
    # LIST16 is then its block-select capacity
    KS16, nh = ks.value // 10, ks.value % 10
    # MFMA products per k-step and tile (csrc/knn_select.hpp, select16_kernel: A_hi x q_hi, plus
    # A_hi x q_lo when kQueryLo = nh == 2 or KS16 >= 4, plus A_lo x q_hi when nh == 2)
    products = 0 if not ks.value else (3 if nh == 2 else (2 if KS16 >= 4 else 1))
    return {"mode": "screened" if ks.value else "exhaustive", "KS16": KS16, "nh": nh,
            "LIST16": lst.value, "split": sp.value, "mfma_products": products}


def knn_issued_mfma_flops(n_cand, n_query, plan):
    """Flops the f16 selection issues on the matrix cores: products x 2 K (K = 16 KS16) per
    32 x 32 tile pair, padded tiles included."""
    tiles = -(-n_query // 32) * -(-n_cand // 32)
    return float(plan["mfma_products"]) * 2 * 16 * plan["KS16"] * 1024 * tiles


class KnnInputCheck:
    """The input validation of a deferred k-NN call (mepol_knn_deferred): the two counts stay
    on the device, copied to pinned host memory in stream order; raise_if_invalid() waits for
    that copy only and raises what mepol_knn would have raised."""

    # Free pinned slots (a pinned allocation per call cost ~1 ms of host time).  A check holds
    # its slot until raise_if_invalid() has read it (or it is collected); with every slot held
    # a new one is allocated, so no check can read another call's counts.
    _free = []
    _lock = threading.Lock()

    def __init__(self, invalid_dev):
        cls = KnnInputCheck
        with cls._lock:
            slot = cls._free.pop() if cls._free else None
        self._host = slot if slot is not None else torch.empty(2, dtype=torch.int32,
                                                               pin_memory=True)
        memcpy_async(self._host, invalid_dev)
        self._event = torch.cuda.Event()
        self._event.record(torch.cuda.current_stream(invalid_dev.device))
        self._dev = invalid_dev
        self._nonfinite = 0

    def raise_if_invalid(self):
        """Raises sklearn's ValueError for a NaN / inf coordinate.  The second count (rows whose
        f32 squared norm overflows) is not an error: those calls were answered by the
        exhaustive f64 scan."""
        from ._lib import MepolInputError

        if self._host is not None:
            self._event.synchronize()
            self._nonfinite = int(self._host[0])
            overflow = int(self._host[1])
            self._release()
            if overflow and not self._nonfinite:
                import warnings

                warnings.warn(f"mepol_knn: {overflow} rows have a squared norm beyond f32; the f16 "
                              "screen was skipped and every query took the exhaustive f64 scan "
                              "(correct, but far slower than the screen)")
        if self._nonfinite:
            raise MepolInputError(f"mepol_knn failed (rc=1001): mepol_knn: Input contains NaN or "
                                  f"infinity ({self._nonfinite} rows)")

    def _release(self):
        """Returns the slot once its copy has landed (never while the copy may still write)."""
        host, self._host = getattr(self, "_host", None), None
        if host is not None:
            self._event.synchronize()
            with KnnInputCheck._lock:
                KnnInputCheck._free.append(host)

    def __del__(self):
        # never block in a finalizer (it runs wherever garbage collection does, and at
        # interpreter shutdown): return the slot only if its copy has already landed, else
        # drop it (the pinned block is freed with the tensor)
        try:
            host, self._host = getattr(self, "_host", None), None
            if host is not None and self._event.query():
                with KnnInputCheck._lock:
                    KnnInputCheck._free.append(host)
        except Exception:
            pass


def knn(cand, kp1, query=None, split=0, want_int64=True, return_fallback=False, defer_check=False):
    """Exact k-NN of `query` rows among `cand` rows (both f32 [*, d] on device), any d and any
    kp1 <= len(cand) (sklearn raises beyond, and so does this: MepolInputError).

    Returns (D f64 [nq, kp1], I int64 [nq, kp1] or None, I32T int32 [kp1, nq]) and, with
    return_fallback, the device int32 count of queries that took the exhaustive path.
    defer_check: no host synchronisation inside the call (mepol_knn_deferred); a KnnInputCheck
    is appended to the result and the caller must call its raise_if_invalid() before using it.
    Replaces NearestNeighbors(k+1).fit(X).kneighbors(X) (src/algorithms/mepol.py:190-192).
    """
    if query is None:
        query = cand
    _require_device(cand, query)
    cand = cand.contiguous().float()
    query = query.contiguous().float()
    nc, d = cand.shape
    nq = query.shape[0]
    if query.shape[1] != d:
        raise ValueError("query/candidate dimension mismatch")
    dev = cand.device
    ws = _ws_or_cached(None, dev, "knn", "knn", nc, nq, d, kp1, split)
    D = torch.empty((nq, kp1), dtype=torch.float64, device=dev)
    I = torch.empty((nq, kp1), dtype=torch.int64, device=dev) if want_int64 else None
    I32T = torch.empty((kp1, nq), dtype=torch.int32, device=dev)
    nfb = torch.zeros(1, dtype=torch.int32, device=dev)
    out = (D, I, I32T) + ((nfb,) if return_fallback else ())
    if defer_check:
        invalid = torch.empty(2, dtype=torch.int32, device=dev)
        call("mepol_knn_deferred", ptr(cand), nc, ptr(query), nq, d, kp1, split, ptr(D), ptr(I),
             ptr(I32T), ptr(nfb), ptr(invalid), ptr(ws), ws.numel(), _stream())
        return out + (KnnInputCheck(invalid),)
    call("mepol_knn", ptr(cand), nc, ptr(query), nq, d, kp1, split, ptr(D), ptr(I), ptr(I32T),
         ptr(nfb), ptr(ws), ws.numel(), _stream())
    return out


def knn_exact(cand, kp1, query=None, want_int64=True):
    """Exhaustive f64 k-NN (every query scanned exactly, no input validation); reference
    semantics, slower: the independent check of knn().  kp1 <= 3072."""
    if query is None:
        query = cand
    _require_device(cand, query)
    cand = cand.contiguous().float()
    query = query.contiguous().float()
    nc, d = cand.shape
    nq = query.shape[0]
    dev = cand.device
    D = torch.empty((nq, kp1), dtype=torch.float64, device=dev)
    I = torch.empty((nq, kp1), dtype=torch.int64, device=dev) if want_int64 else None
    I32T = torch.empty((kp1, nq), dtype=torch.int32, device=dev)
    call("mepol_knn_exact", ptr(cand), nc, ptr(query), nq, d, kp1, ptr(D), ptr(I), ptr(I32T),
         None, _stream())
    return D, I, I32T


def iw_forward(logp_t, logp_b, offsets, n_particles, normalize=True, w_out=None, u_out=None,
               ts_out=None):
    """u = exp(segmented cumsum(logp_t - logp_b)); w = u / sum(u).

    logp_t/logp_b: f64 [nt, T_stride]; offsets: int64 [nt+1] particle offsets.
    Returns (u [N], traj_sum [nt], w [N] or None, U 0-d or None).
    """
    _require_device(logp_t, logp_b, offsets)
    nt, Ts = logp_t.shape
    dev = logp_t.device
    lt = logp_t.contiguous()
    lb = logp_b.contiguous()
    u = u_out if u_out is not None else torch.empty(n_particles, dtype=torch.float64, device=dev)
    ts = ts_out if ts_out is not None else torch.empty(nt, dtype=torch.float64, device=dev)
    w = (w_out if w_out is not None else torch.empty(n_particles, dtype=torch.float64,
                                                     device=dev)) if normalize else None
    U = torch.empty((), dtype=torch.float64, device=dev) if normalize else None
    call("mepol_iw_forward", ptr(lt), ptr(lb), nt, Ts, ptr(offsets), n_particles, ptr(u), ptr(ts),
         ptr(w), ptr(U), _stream())
    return u, ts, w, U


def iw_normalize(u, U, out=None):
    w = out if out is not None else torch.empty_like(u)
    call("mepol_iw_normalize", ptr(u), ptr(U), u.numel(), ptr(w), _stream())
    return w


def entropy_forward(w, idxT, D, k, ns, G, B, eps, n_w=None, g_out=None, out4=None, vals=None):
    """Fused compute_entropy + compute_kl forward.

    Returns (out4 f64[4] = {H, KL_unclamped, sum_term, sum_klterm}, W [n], g [n]).  With `vals`
    (f64[2]) and `out4` given, out4 is updated in place and vals = {out4[0] on entry, new KL}.
    """
    _require_device(w, idxT, D)
    n = D.shape[0]
    kp1 = D.shape[1]
    dev = w.device
    if n_w is None:
        n_w = w.numel()
    nparts = _lib.load().mepol_entropy_partials_size(n)
    partials = torch.empty(max(2 * nparts, 2), dtype=torch.float64, device=dev)
    W = torch.empty(n, dtype=torch.float64, device=dev)
    g = g_out if g_out is not None else torch.empty(n, dtype=torch.float64, device=dev)
    if vals is not None:
        assert out4 is not None
        call("mepol_entropy_forward_emit", ptr(w.contiguous()), ptr(idxT), ptr(D.contiguous()), n,
             n_w, k, kp1, float(ns), float(G), float(B), float(eps), ptr(W), ptr(g),
             ptr(partials), ptr(out4), ptr(vals), _stream())
        return out4, W, g
    out4 = out4 if out4 is not None else torch.empty(4, dtype=torch.float64, device=dev)
    call("mepol_entropy_forward", ptr(w.contiguous()), ptr(idxT), ptr(D.contiguous()), n, n_w, k,
         kp1, float(ns), float(G), float(B), float(eps), ptr(W), ptr(g), ptr(partials), ptr(out4),
         _stream())
    return out4, W, g


def iw_normalize_gathered(xu_all, world, n, nt, w_out):
    """w_out [world n] <- the all-gathered [u | per-trajectory sums] blocks (world x (n + nt))
    normalised by the fixed-order sum of all ranks' trajectory sums."""
    call("mepol_iw_normalize_gathered", ptr(xu_all), world, n, nt, ptr(w_out), _stream())
    return w_out


def sharded_emit(x_all, world, stride, off, B, n_global, sums_cur, vals):
    """vals <- (B - sums_cur[0], rank-order sum of x_all[r, off + 1] / n_global);
    sums_cur <- the rank-order sums of x_all[r, off], x_all[r, off + 1]."""
    call("mepol_sharded_emit", ptr(x_all), world, stride, off, float(B), n_global, ptr(sums_cur),
         ptr(vals), _stream())


def csr_build(idxT, k, n_own, col_offset=0, row_offset=0, nq=None):
    """CSR transpose of the first k rows of idxT ([>=k, nq]) for ids [col_offset, +n_own)."""
    _require_device(idxT)
    if nq is None:
        nq = idxT.shape[1]
    dev = idxT.device
    ws = _ws_or_cached(None, dev, "csr", "csr", nq, k, n_own)
    off = torch.empty(n_own + 1, dtype=torch.int32, device=dev)
    rows = torch.empty(max(nq * k, 1), dtype=torch.int32, device=dev)
    call("mepol_csr_build", ptr(idxT), nq, k, col_offset, n_own, row_offset, ptr(off), ptr(rows),
         ptr(ws), ws.numel(), _stream())
    return off, rows


def entropy_gamma_nparts(n_own):
    """Block partials entropy_gamma returns (csrc/entropy.hip: one per 256-thread block of
    kGammaLanes lanes per particle, at most kGammaMaxBlocks)."""
    return int(_lib.load().mepol_entropy_gamma_partials_size(n_own))


def entropy_gamma(g, w_own, csr_off, csr_rows):
    n_own = w_own.numel()
    dev = w_own.device
    gamma = torch.empty(n_own, dtype=torch.float64, device=dev)
    nparts = entropy_gamma_nparts(n_own)
    partials = torch.empty(max(nparts, 1), dtype=torch.float64, device=dev)
    call("mepol_entropy_gamma", ptr(g), ptr(w_own), ptr(csr_off), ptr(csr_rows), n_own,
         ptr(gamma), ptr(partials), _stream())
    return gamma, partials, nparts


def entropy_reverse_scan(gamma, w, partials, nparts, offsets, nt, T_stride, grad_H, S_ext=None):
    grad = torch.empty((nt, T_stride), dtype=torch.float64, device=w.device)
    call("mepol_entropy_reverse_scan", ptr(gamma), ptr(w), ptr(partials), nparts, ptr(S_ext),
         ptr(offsets), nt, T_stride, ptr(grad_H), ptr(grad), _stream())
    return grad


def head_forward(z, Wm, bm, log_std, act, bz=None, mu_out=None, logp_out=None):
    """Fused Gaussian head: (mu [n, a], logp [n]) from the last pre-activation z (+ bias bz)."""
    n, h = z.shape
    a = Wm.shape[0]
    mu = mu_out if mu_out is not None else torch.empty((n, a), dtype=torch.float64, device=z.device)
    logp = logp_out if logp_out is not None else torch.empty(n, dtype=torch.float64,
                                                             device=z.device)
    call("mepol_head_forward", ptr(z), n, h, ptr(bz), ptr(Wm), ptr(bm), ptr(log_std), ptr(act), a,
         ptr(mu), ptr(logp), _stream())
    return mu, logp


def head_backward(grad_logp, z, Wm, log_std, act, mu, bz=None, need_dz=True, ws=None,
                  outs=None, reduce_stream=None, defer_reduce=False):
    """Returns (dz or None, dWm, dbm, dlog_std, dbz or None).  `ws`: caller-owned scratch
    (head_workspace); default: the per-stream eager cache.  `outs`: optional (dWm, dbm,
    dlog_std, dbz) tensors to write instead of fresh ones.  `reduce_stream`: the parameter
    gradients' two reduce kernels run there (ordered after the row kernel on the current
    stream, mepol_head_backward_phase), dz is ready on the current stream; the caller joins
    reduce_stream before reading dWm / dbm / dlog_std / dbz (same bits either way).
    `defer_reduce`: only the row kernel runs now; a sixth return value finish() launches the
    reduces on the then-current stream, which must be ordered after this one and before the
    workspace is reused."""
    n, h = z.shape
    a = Wm.shape[0]
    dev = z.device
    ws = _ws_or_cached(ws, dev, "head", "head", n, h, a)
    dz = torch.empty_like(z) if need_dz else None
    if outs is not None:
        dWm, dbm, dls, dbz = outs
        assert all(t is None or t.is_contiguous() for t in outs)
    else:
        dWm = torch.empty_like(Wm)
        dbm = torch.empty(a, dtype=torch.float64, device=dev)
        dls = torch.empty(a, dtype=torch.float64, device=dev)
        dbz = torch.empty(h, dtype=torch.float64, device=dev) if bz is not None else None
    args = (ptr(grad_logp), ptr(z), n, h, ptr(bz), ptr(Wm), ptr(log_std), ptr(act), ptr(mu), a,
            ptr(dz), ptr(dWm), ptr(dbm), ptr(dls), ptr(dbz), ptr(ws), ws.numel())
    if defer_reduce:
        call("mepol_head_backward_phase", *args, 1, _stream())
        return dz, dWm, dbm, dls, dbz, lambda: call("mepol_head_backward_phase", *args, 2,
                                                    _stream())
    if reduce_stream is None:
        call("mepol_head_backward", *args, _stream())
        return dz, dWm, dbm, dls, dbz
    call("mepol_head_backward_phase", *args, 1, _stream())
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream())
    reduce_stream.wait_event(done)
    with torch.cuda.stream(reduce_stream):
        call("mepol_head_backward_phase", *args, 2, _stream())
    if not torch.cuda.is_current_stream_capturing():  # a graph keeps its buffers alive
        for t in (dWm, dbm, dls, dbz, ws):
            if t is not None:
                t.record_stream(reduce_stream)
    return dz, dWm, dbm, dls, dbz


POLICY_FWD_MAX_IN = 64
POLICY_FWD_MAX_H1 = 320


def policy_forward_ok(in_features, hidden1):
    return in_features <= POLICY_FWD_MAX_IN and hidden1 <= POLICY_FWD_MAX_H1


def h1_mask_buffer(n, hidden0, device):
    """relu'(h1) bit mask of policy_forward(mask_out=...): [n, ceil(hidden0 / 16)] int16."""
    return torch.empty((n, (hidden0 + 15) // 16), dtype=torch.int16, device=device)


def policy_forward_plan(n, in_features, hidden0, hidden1):
    """{"row_tile"}: the rows per workgroup policy_forward(row_tile=0) takes for its z2 / head
    kernel at n rows (host only: mepol_policy_forward_plan_info)."""
    tile = ctypes.c_int()
    call("mepol_policy_forward_plan_info", n, in_features, hidden0, hidden1, ctypes.byref(tile))
    return {"row_tile": tile.value}


def policy_forward(x, W1, b1, W2, b2, Wm, bm, log_std, act, h1_out=None, z2_out=None,
                   mu_out=None, logp_out=None, mask_out=None, row_tile=0):
    """One-kernel forward of the two-hidden-layer Gaussian policy: returns (h1, z2, mu, logp)
    with h1 = relu(x W1^T + b1), z2 = h1 W2^T (pre-bias), mu = relu(z2 + b2) Wm^T + bm and
    logp = sum_a log N(act | mu, exp(log_std) + 1e-7).  With mask_out (h1_mask_buffer) the
    kernel also writes relu'(h1) as bits for dh1_layer1_backward(mask=...).  row_tile: rows per
    workgroup of the z2 / head kernel, 0 = chosen from n (policy_forward_plan), or 64 / 32 / 16
    (the same bits for each; anything else raises MepolInputError)."""
    n, f = x.shape
    h0, h1w, a = W1.shape[0], W2.shape[0], Wm.shape[0]
    dev = x.device

    def buf(t, shape):
        return t if t is not None else torch.empty(shape, dtype=torch.float64, device=dev)

    h1 = buf(h1_out, (n, h0))
    z2 = buf(z2_out, (n, h1w))
    mu = buf(mu_out, (n, a))
    logp = buf(logp_out, (n,))
    if mask_out is not None:
        assert mask_out.shape == (n, (h0 + 15) // 16) and mask_out.dtype == torch.int16
        assert mask_out.is_contiguous()
    call("mepol_policy_forward_tiled", ptr(x), n, f, ptr(W1), ptr(b1), h0, ptr(W2), ptr(b2), h1w,
         ptr(Wm), ptr(bm), ptr(log_std), ptr(act), a, ptr(h1), ptr(z2), ptr(mu), ptr(logp),
         ptr(mask_out), int(row_tile), _stream())
    return h1, z2, mu, logp


DH1_L1_MAX_IN = 63


def dh1_layer1_ok(in_features, hidden1):
    return in_features <= DH1_L1_MAX_IN and hidden1 % 2 == 0


def dh1_layer1_backward(dz2, W2t, h1, x, ws=None, dW_out=None, db_out=None, mask=None,
                        w2=None, form="auto"):
    """(dW1, db1) of h1 = relu(x W1^T + b1) from dz2 = dL/dz2 [n, h1w] and W2t = W2^T
    [h0, h1w]: dh1 = dz2 W2 is reduced on chip (csrc/gemm.hip), never written.  With `w2`
    (W2 as stored, [h1w, h0]; needs `mask`) W2t is not read and may be None: the kernel
    transposes W2's tiles itself (mepol_dh1_layer1_backward_w2).  form (mask forms only): "auto",
    or "lds" / "direct" to name the kernel (dh1_layer1_plan; the same bits either way)."""
    n, k = dz2.shape
    f = x.shape[1]
    if w2 is not None:
        h0 = w2.shape[1]
        assert mask is not None and w2.shape[0] == k and w2.is_contiguous() and dz2.is_contiguous()
    else:
        h0 = W2t.shape[0]
        assert W2t.shape[1] == k and h1.shape == (n, h0) and dz2.is_contiguous() and W2t.is_contiguous()
    ws = _ws_or_cached(ws, x.device, "dh1l1", "dh1_layer1", n, h0, f)
    dW = dW_out if dW_out is not None else torch.empty((h0, f), dtype=torch.float64,
                                                      device=x.device)
    db = db_out if db_out is not None else torch.empty(h0, dtype=torch.float64, device=x.device)
    assert dW.is_contiguous() and db.is_contiguous()
    if form != "auto":
        assert mask is not None and mask.shape == (n, (h0 + 15) // 16)
        assert mask.dtype == torch.int16
        call("mepol_dh1_layer1_backward_form", ptr(dz2), n, k, ptr(w2 if w2 is not None else W2t),
             h0, ptr(mask), ptr(x), f, ptr(dW), ptr(db), ptr(ws), ws.numel(),
             int(w2 is not None), DH1_FORMS[form], _stream())
    elif w2 is not None:
        assert mask.shape == (n, (h0 + 15) // 16) and mask.dtype == torch.int16
        call("mepol_dh1_layer1_backward_w2", ptr(dz2), n, k, ptr(w2), h0, ptr(mask), ptr(x), f,
             ptr(dW), ptr(db), ptr(ws), ws.numel(), _stream())
    elif mask is None:
        call("mepol_dh1_layer1_backward", ptr(dz2), n, k, ptr(W2t), h0, ptr(h1), ptr(x), f,
             ptr(dW), ptr(db), ptr(ws), ws.numel(), _stream())
    else:  # relu'(h1) from the forward's bit mask (policy_forward(mask_out=...))
        assert mask.shape == (n, (h0 + 15) // 16) and mask.dtype == torch.int16
        call("mepol_dh1_layer1_backward_masked", ptr(dz2), n, k, ptr(W2t), h0, ptr(mask),
             ptr(x), f, ptr(dW), ptr(db), ptr(ws), ws.numel(), _stream())
    return dW, db


DH1_FORMS = {"auto": 0, "lds": 1, "direct": 2}


def dh1_layer1_plan(n, k, hidden0, in_features, mask=True, w2=False, form="auto"):
    """Which kernel dh1_layer1_backward launches at these sizes (host only:
    mepol_dh1_layer1_plan_info): {"form": "direct" (operands from L2 into registers) or "lds",
    "nh", "row_blocks", "col_tiles", "threads", "lds_bytes", "waves_per_block", "rows_per_wave",
    "record_doubles", "group_offset", "ws_bytes"}.  mask: the bit-mask forms; w2: W2 as stored;
    form: as asked of dh1_layer1_backward."""
    names = ("form", "nh", "row_blocks", "col_tiles", "threads", "lds_bytes", "waves_per_block",
             "rows_per_wave")
    ints = {k_: ctypes.c_int() for k_ in names}
    rec = ctypes.c_int64()
    off, wsb = ctypes.c_size_t(), ctypes.c_size_t()
    call("mepol_dh1_layer1_plan_info", n, k, hidden0, in_features, int(bool(mask)), int(bool(w2)),
         DH1_FORMS[form], *[ctypes.byref(ints[k_]) for k_ in names], ctypes.byref(rec), ctypes.byref(off),
         ctypes.byref(wsb))
    plan = {k_: v.value for k_, v in ints.items()}
    plan["form"] = "direct" if plan["form"] == 1 else "lds"
    plan.update(record_doubles=rec.value, group_offset=off.value, ws_bytes=wsb.value)
    return plan


def weight_grad_workspace(n, out_features, in_features, device):
    """Scratch of weight_grad (its K-slices' partial blocks), owned by the caller."""
    return _own_workspace(device, "weight_grad", n, out_features, in_features)


def weight_grad_plan(n, out_features, in_features):
    """The launch plan of weight_grad at these sizes (host only: mepol_weight_grad_plan_info):
    {"nob", "nib", "fol", "Sf", "Ss", "rows_f", "rows_s", "grid8"} and the slice -> XCD map
    "fend", "send", "fbase", "sbase" (lists of 8), as csrc/wgrad.hip's Plan describes them."""
    ints = {k: ctypes.c_int() for k in ("nob", "nib", "fol", "Sf", "Ss", "grid8")}
    rows = {k: ctypes.c_int64() for k in ("rows_f", "rows_s")}
    maps = {k: (ctypes.c_int * 8)() for k in ("fend", "send", "fbase", "sbase")}
    call("mepol_weight_grad_plan_info", n, out_features, in_features,
         *[ctypes.byref(ints[k]) for k in ("nob", "nib", "fol", "Sf", "Ss")],
         ctypes.byref(rows["rows_f"]), ctypes.byref(rows["rows_s"]), ctypes.byref(ints["grid8"]),
         *[maps[k] for k in ("fend", "send", "fbase", "sbase")])
    plan = {k: v.value for k, v in {**ints, **rows}.items()}
    plan.update({k: list(v) for k, v in maps.items()})
    return plan


def weight_grad(dy, x, out=None, ws=None):
    """dW = dy^T x for dy [n, out] and x [n, in] (f64, row-major): the weight gradient of a
    Linear layer over a tall batch (csrc/wgrad.hip: split-K on the f64 matrix cores, fixed-order
    sum over the K-slices)."""
    n, o = dy.shape
    i = x.shape[1]
    assert x.shape[0] == n and dy.is_contiguous() and x.is_contiguous()
    assert dy.dtype == torch.float64 and x.dtype == torch.float64
    if ws is None:
        ws = weight_grad_workspace(n, o, i, dy.device)
    dW = out if out is not None else torch.empty((o, i), dtype=torch.float64, device=dy.device)
    assert dW.is_contiguous() and dW.shape == (o, i)
    call("mepol_weight_grad", ptr(dy), n, o, ptr(x), i, ptr(dW), ptr(ws), ws.numel(), _stream())
    return dW


def hidden_backward_workspace(n, in_features, device):
    """Scratch of hidden_backward (its row blocks' column sums), owned by the caller."""
    return _own_workspace(device, "hidden_backward", n, in_features)


def hidden_backward(dz_out, W, h_in, ws=None, dz_out_buf=None, db_out=None):
    """(dz_in, db_in) of a hidden layer h_out = relu(h_in W^T + b) from dz_out = dL/d(its
    pre-activation) [n, out]: dz_in = (dz_out W) * (h_in > 0) [n, in], the gradient at the
    previous layer's pre-activation, and db_in = dz_in.sum(0), that layer's bias gradient
    (csrc/gemm.hip: W read as stored on the f64 matrix cores, fixed-order column sums).
    `dz_out_buf` / `db_out`: optional tensors the results are written into."""
    n, o = dz_out.shape
    i = W.shape[1]
    assert W.shape[0] == o and h_in.shape == (n, i)
    assert dz_out.is_contiguous() and W.is_contiguous() and h_in.is_contiguous()
    assert dz_out.dtype == torch.float64 and W.dtype == torch.float64 and h_in.dtype == torch.float64
    ws = _ws_or_cached(ws, dz_out.device, "hidbwd", "hidden_backward", n, i)
    dz = dz_out_buf if dz_out_buf is not None else torch.empty((n, i), dtype=torch.float64,
                                                                device=dz_out.device)
    db = db_out if db_out is not None else torch.empty(i, dtype=torch.float64,
                                                       device=dz_out.device)
    assert dz.is_contiguous() and dz.shape == (n, i) and db.is_contiguous() and db.numel() == i
    call("mepol_hidden_backward", ptr(dz_out), n, o, ptr(W), ptr(h_in), i, ptr(dz), ptr(db),
         ptr(ws), ws.numel(), _stream())
    return dz, db


def _f64_rows(name, *ts):
    for t in ts:
        if t is not None and (t.dtype != torch.float64 or not t.is_contiguous()):
            raise ValueError(f"{name} needs contiguous f64 tensors")


def layer_tangent(x, dW, db, h, out=None):
    """Tangent of the input layer h = relu(x W^T + b) along (dW, db): (x dW^T + db) * (h > 0)
    (csrc/mlp.hip; in_features <= 64)."""
    _require_device(x, dW, db, h, out)
    n, f = x.shape
    o = dW.shape[0]
    if dW.shape != (o, f) or db.shape != (o,) or h.shape != (n, o):
        raise ValueError("layer_tangent: x [n, in], dW [out, in], db [out], h [n, out]")
    t = out if out is not None else torch.empty((n, o), dtype=torch.float64, device=x.device)
    _f64_rows("layer_tangent", x, dW, db, h, t)
    assert t.shape == (n, o)
    call("mepol_layer_tangent", ptr(x), n, f, ptr(dW), ptr(db), o, ptr(h), ptr(t), _stream())
    return t


def hidden_tangent(t_in, h_in, W, dW, db, mask_src, mask_bias=None, out=None, variant=0):
    """Tangent of a hidden layer h_out = relu(h_in W^T + b) along (dW, db) given the tangent t_in
    of h_in: (t_in W^T + h_in dW^T + db) * (mask_src + mask_bias > 0) on the f64 matrix cores
    (csrc/gemm.hip; both products in the same accumulators).  mask_src = h_out with no
    mask_bias, or the pre-bias z with mask_bias = b.  `variant`: gemm_nt's tilings."""
    _require_device(t_in, h_in, W, dW, db, mask_src, mask_bias, out)
    n, k = t_in.shape
    m = W.shape[0]
    if (h_in.shape != (n, k) or W.shape != (m, k) or dW.shape != (m, k) or db.shape != (m,)
            or mask_src.shape != (n, m) or (mask_bias is not None and mask_bias.shape != (m,))):
        raise ValueError("hidden_tangent: t_in, h_in [n, k], W, dW [m, k], db [m], mask_src "
                         "[n, m], mask_bias [m]")
    t = out if out is not None else torch.empty((n, m), dtype=torch.float64, device=t_in.device)
    _f64_rows("hidden_tangent", t_in, h_in, W, dW, db, mask_src, mask_bias, t)
    assert t.shape == (n, m)
    call("mepol_hidden_tangent", ptr(t_in), ptr(h_in), n, k, ptr(W), ptr(dW), ptr(db), m,
         ptr(mask_src), ptr(mask_bias), ptr(t), int(variant), _stream())
    return t


def mean_tangent(t, z, Wm, dWm, dbm, scale, bz=None, out=None):
    """c = scale * (t Wm^T + relu(z + bz) dWm^T + dbm): the mean layer's tangent along (tangent t
    of the last hidden layer, dWm, dbm), scaled per action by the device vector `scale`
    (csrc/head.hip; hidden <= 512, action_dim <= 32)."""
    _require_device(t, z, Wm, dWm, dbm, scale, bz, out)
    n, h = z.shape
    a = Wm.shape[0]
    if (t.shape != (n, h) or Wm.shape != (a, h) or dWm.shape != (a, h) or dbm.shape != (a,)
            or scale.shape != (a,) or (bz is not None and bz.shape != (h,))):
        raise ValueError("mean_tangent: t, z [n, hidden], Wm, dWm [a, hidden], dbm, scale [a], "
                         "bz [hidden]")
    c = out if out is not None else torch.empty((n, a), dtype=torch.float64, device=z.device)
    _f64_rows("mean_tangent", t, z, Wm, dWm, dbm, scale, bz, c)
    assert c.shape == (n, a)
    call("mepol_mean_tangent", ptr(t), ptr(z), n, h, ptr(bz), ptr(Wm), ptr(dWm), ptr(dbm),
         ptr(scale), a, ptr(c), _stream())
    return c


def mean_backward_workspace(n, hidden, a, device):
    """A caller-owned scratch buffer for mean_backward at these sizes."""
    return _own_workspace(device, "mean_backward", n, hidden, a)


def mean_backward(c, z, Wm, bz=None, need_dz=True, ws=None, dz_out=None, outs=None):
    """Mean-layer backward from a cotangent c [n, a] on mu: returns (dz or None, dWm, dbm, dbz or
    None) with dWm = c^T relu(z + bz), dbm = c.sum(0), dz = (c Wm) * (z + bz > 0), dbz = dz.sum(0)
    (csrc/head.hip; fixed-order row sums).  `outs`: optional (dWm, dbm, dbz) tensors to write;
    `dz_out`: optional dz buffer."""
    _require_device(c, z, Wm, bz, dz_out)
    n, h = z.shape
    a = Wm.shape[0]
    if c.shape != (n, a) or Wm.shape != (a, h) or (bz is not None and bz.shape != (h,)):
        raise ValueError("mean_backward: c [n, a], z [n, hidden], Wm [a, hidden], bz [hidden]")
    dev = z.device
    ws = _ws_or_cached(ws, dev, "meanbwd", "mean_backward", n, h, a)
    dz = (dz_out if dz_out is not None else torch.empty_like(z)) if need_dz else None
    if outs is not None:
        dWm, dbm, dbz = outs
    else:
        dWm = torch.empty((a, h), dtype=torch.float64, device=dev)
        dbm = torch.empty(a, dtype=torch.float64, device=dev)
        dbz = torch.empty(h, dtype=torch.float64, device=dev) if bz is not None else None
    _f64_rows("mean_backward", c, z, Wm, bz, dz, dWm, dbm, dbz)
    assert dWm.shape == (a, h) and dbm.numel() == a and (dbz is None or dbz.numel() == h)
    assert dz is None or dz.shape == (n, h)
    call("mepol_mean_backward", ptr(c), ptr(z), n, h, ptr(bz), ptr(Wm), a, ptr(dz), ptr(dWm),
         ptr(dbm), ptr(dbz), ptr(ws), ws.numel(), _stream())
    return dz, dWm, dbm, dbz


GEMM_NT_CUS = 256          # gfx950
GEMM_NT_KEEP_ROWS = 16384  # from here on variant 0 always (the large-batch path, as measured)


def gemm_nt_variant(n, m):
    """The gemm_nt tiling of the deep policy's layers for an [n, m] output: variant 0 (128 x 160
    tiles) when its grid reaches the CU count, and for every n >= 16384; variant 2 (64 x 160,
    twice the workgroups) for a smaller batch whose variant-0 grid would leave CUs idle."""
    if n >= GEMM_NT_KEEP_ROWS:
        return 0
    tiles = -(-n // 128) * -(-m // 160)
    return 0 if tiles >= GEMM_NT_CUS else 2


def gemm_nt(A, B, bias=None, relu=False, out=None, variant=0):
    """act(A B^T + bias) on the f64 matrix cores: A [n, k], B [m, k] (row-major, k even)."""
    n, k = A.shape
    m = B.shape[0]
    assert B.shape[1] == k and A.stride(1) == 1 and B.stride(1) == 1
    C = out if out is not None else torch.empty((n, m), dtype=torch.float64, device=A.device)
    call("mepol_gemm_nt", ptr(A), n, k, A.stride(0), ptr(B), m, B.stride(0), ptr(bias),
         int(relu), ptr(C), C.stride(0), variant, _stream())
    return C


def layer_forward(x, W, b, out=None):
    """h = relu(x W^T + b) for the policy's input layer (in_features <= 64)."""
    n, f = x.shape
    h = out if out is not None else torch.empty((n, W.shape[0]), dtype=torch.float64,
                                                device=x.device)
    call("mepol_layer_forward", ptr(x), n, f, ptr(W), ptr(b), W.shape[0], ptr(h), _stream())
    return h


def layer_backward(dh, h, x, ws=None, dW_out=None, db_out=None):
    """(dW, db) of h = relu(x W^T + b) from dL/dh and the forward output h.  `ws`: caller-owned
    scratch (layer_workspace); default: the per-stream eager cache.  `dW_out` / `db_out`:
    optional contiguous tensors the results are written into."""
    n, f = x.shape
    out = h.shape[1]
    ws = _ws_or_cached(ws, x.device, "layer", "layer", n, f, out)
    dW = dW_out if dW_out is not None else torch.empty((out, f), dtype=torch.float64,
                                                      device=x.device)
    db = db_out if db_out is not None else torch.empty(out, dtype=torch.float64, device=x.device)
    assert dW.is_contiguous() and dW.shape == (out, f) and db.is_contiguous() and db.numel() == out
    call("mepol_layer_backward", ptr(dh), ptr(h), ptr(x), n, f, out, ptr(dW), ptr(db), ptr(ws),
         ws.numel(), _stream())
    return dW, db


def optim_step(kind, params, grads, exp_avg, exp_avg_sq, scalars, snapshot=None):
    """In-place Adam (kind 0) / RMSprop (kind 1) update of f64 tensors; scalars is a device f64
    tensor (see include/mepol_amd.h, mepol_optim_step).  snapshot = (params_snap, exp_avg_snap,
    exp_avg_sq_snap) lists (entries may be None) receive the values from before the update."""
    n = len(params)
    arr = ctypes.c_void_p * n
    snaps = list(snapshot) if snapshot is not None else [None, None, None]
    for t in (list(params) + list(grads) + list(exp_avg_sq) + list(exp_avg or [])
              + [x for lst in snaps if lst is not None for x in lst]):
        if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("optim_step needs contiguous f64 device tensors")
    for lst in snaps:
        if lst is not None and (len(lst) != n or any(
                a.numel() != b.numel() for a, b in zip(lst, params))):
            raise ValueError("optim_step: snapshot tensors must match the parameters")
    sizes = (ctypes.c_int64 * n)(*[t.numel() for t in params])
    m = arr(*[t.data_ptr() for t in exp_avg]) if exp_avg is not None else None
    sp = [arr(*[t.data_ptr() for t in lst]) if lst is not None else None for lst in snaps]
    call("mepol_optim_step_snapshot", kind, n, arr(*[t.data_ptr() for t in params]),
         arr(*[t.data_ptr() for t in grads]), m, arr(*[t.data_ptr() for t in exp_avg_sq]),
         sizes, ptr(scalars), sp[0], sp[1], sp[2], _stream())


CRITIC_FIT_MAX_FEATURES, CRITIC_FIT_MAX_WIDTH, CRITIC_FIT_MAX_BATCH = 16, 64, 64


def critic_fit_plan(nf, h0, h1, batch):
    """{threads, lds_bytes, accepted} of mepol_critic_fit at this shape (host only)."""
    t, l, ok = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    call("mepol_critic_fit_plan_info", int(nf), int(h0), int(h1), int(batch), ctypes.byref(t),
         ctypes.byref(l), ctypes.byref(ok))
    return {"threads": t.value, "lds_bytes": l.value, "accepted": bool(ok.value)}


def adam_step_scalars(lr, betas, first_step, n_steps):
    """[n_steps, 2] f64 host tensor of (lr / bias_correction1, sqrt(bias_correction2)) for step
    numbers first_step .. first_step + n_steps - 1, in Python f64 as torch.optim.Adam computes
    them (the convention of optim_step's scalars)."""
    beta1, beta2 = betas
    rows = []
    for k in range(int(n_steps)):
        step = float(first_step + k)
        rows.append((lr / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5))
    return torch.tensor(rows, dtype=torch.float64).reshape(int(n_steps), 2)


def critic_fit(states, targets, index, batch, params, exp_avg, exp_avg_sq, lr, betas=(0.9, 0.999),
               eps=1e-8, first_step=1, loss_out=None):
    """n_steps = index.numel() // batch Adam steps of the critic's mini-batch fit in one launch
    (mepol_critic_fit): step s fits rows index[s * batch : (s + 1) * batch] of states [N, nf] /
    targets [N] to loss mean((v(x) - t)^2).  params = [W1, b1, W2, b2, W3, b3] of Linear(nf, h0)
    -> ReLU -> Linear(h0, h1) -> ReLU -> Linear(h1, 1), exp_avg / exp_avg_sq their Adam moments:
    contiguous f64 device tensors, updated in place.  index is int32 on the device with entries
    in [0, N).  first_step is the number of the first step (torch's state['step'] + 1): it sets
    the bias corrections.  Returns loss_out [n_steps]: each step's loss before its update."""
    params, exp_avg, exp_avg_sq = list(params), list(exp_avg), list(exp_avg_sq)
    _require_device(states, targets, index, loss_out, *params, *exp_avg, *exp_avg_sq)
    if len(params) != 6 or len(exp_avg) != 6 or len(exp_avg_sq) != 6:
        raise ValueError("critic_fit: six parameter tensors and their moments are needed")
    for t in [states, targets] + params + exp_avg + exp_avg_sq:
        if t.dtype != torch.float64 or not t.is_contiguous() or t.device != states.device:
            raise ValueError("critic_fit needs contiguous f64 tensors on one device")
    if index.dtype != torch.int32 or not index.is_contiguous() or index.device != states.device:
        raise ValueError("critic_fit: index must be a contiguous int32 tensor on the device")
    if states.dim() != 2 or targets.dim() != 1 or targets.shape[0] != states.shape[0]:
        raise ValueError("critic_fit: states [N, nf] and targets [N] are needed")
    n, nf = states.shape
    W1, b1, W2, b2, W3, b3 = params
    h0, h1 = W1.shape[0], W2.shape[0]
    shapes = [(h0, nf), (h0,), (h1, h0), (h1,), (1, h1), (1,)]
    for lst in (params, exp_avg, exp_avg_sq):
        if [tuple(t.shape) for t in lst] != shapes:
            raise ValueError(f"critic_fit: tensors of shapes {shapes} are needed, in that order")
    batch = int(batch)
    # the shape limits (batch < 1 among them) are the library's to refuse, with its message
    n_steps = index.numel() // batch if batch > 0 else 1
    if n_steps < 1 or (batch > 0 and index.numel() % batch):
        raise ValueError("critic_fit: index must hold a whole number (>= 1) of mini-batches")
    dev = states.device
    scal = adam_step_scalars(lr, betas, first_step, n_steps).to(dev)
    if loss_out is None:
        loss_out = torch.empty(n_steps, dtype=torch.float64, device=dev)
    elif (loss_out.dtype != torch.float64 or not loss_out.is_contiguous()
          or loss_out.numel() != n_steps):
        raise ValueError("critic_fit: loss_out must be a contiguous f64 tensor of n_steps")
    arr = ctypes.c_void_p * 6
    call("mepol_critic_fit", ptr(states), ptr(targets), n, ptr(index), n_steps, batch, nf, h0, h1,
         arr(*[t.data_ptr() for t in params]), arr(*[t.data_ptr() for t in exp_avg]),
         arr(*[t.data_ptr() for t in exp_avg_sq]), ptr(scal), float(betas[0]), float(betas[1]),
         float(eps), ptr(loss_out), _stream())
    return loss_out


def step_mountaincar(state, action):
    """In-place batched MountainCar step: state f64 [n,2], action f64 [n, a>=1]."""
    _require_device(state, action)
    call("mepol_step_mountaincar", ptr(state), ptr(action), state.shape[0], action.stride(0),
         _stream())
    return state


def step_gridworld(state, action):
    """In-place batched GridWorld step: state f32 [n,2], action f64 [n,2]."""
    _require_device(state, action)
    call("mepol_step_gridworld", ptr(state), ptr(action.contiguous()), state.shape[0], _stream())
    return state


MAZE = 2  # the kernels' env_id of a box maze (envs/maze.py); 0 MountainCar, 1 GridWorld


def maze_struct(maze):
    """The C ABI's mepol_maze of a BoxMazeContinuous (or any object with its `bounds`,
    `max_delta` and `walls`).  The library validates it again before every launch."""
    walls = list(maze.walls)
    if len(walls) > _lib.MAZE_MAX_WALLS:
        raise ValueError(f"a maze of {len(walls)} walls: the kernels take at most "
                         f"{_lib.MAZE_MAX_WALLS}")
    m = _lib.Maze()
    m.xlo, m.xhi, m.ylo, m.yhi = (float(v) for v in maze.bounds)
    m.max_delta = float(maze.max_delta)
    m.n_walls = len(walls)
    for w, box in enumerate(walls):
        for k in range(4):
            m.walls[w][k] = float(box[k])
    return m


def _maze_arg(who, env_id, maze):
    """The maze entry points' first argument when env_id is MAZE, else None.  `maze=` belongs to
    env_id 2 and only there: anything else raises."""
    if env_id == MAZE:
        if maze is None:
            raise ValueError(f"{who}: env_id 2 (box maze) needs maze=")
        return ctypes.byref(maze if isinstance(maze, _lib.Maze) else maze_struct(maze))
    if maze is not None:
        raise ValueError(f"{who}: maze= goes with env_id 2 only (got env_id {env_id})")
    return None


def step_maze(state, action, maze):
    """In-place batched box-maze step: state f32 [n,2], action f64 [n,2]."""
    _require_device(state, action)
    call("mepol_step_maze", _maze_arg("step_maze", MAZE, maze), ptr(state),
         ptr(action.contiguous()), state.shape[0], _stream())
    return state


def rollout_step(env_id, env_f64, env_f32, mean, noise, log_std, t, T, states_rec, actions_rec,
                 policy_in, maze=None):
    n, a_dim = mean.shape
    mz = _maze_arg("rollout_step", env_id, maze)
    if mz is not None:
        call("mepol_rollout_step_maze", mz, ptr(env_f32), ptr(mean), ptr(noise), ptr(log_std), n,
             a_dim, t, T, ptr(states_rec), ptr(actions_rec), ptr(policy_in), _stream())
        return
    call("mepol_rollout_step", env_id, ptr(env_f64), ptr(env_f32), ptr(mean), ptr(noise),
         ptr(log_std), n, a_dim, t, T, ptr(states_rec), ptr(actions_rec), ptr(policy_in),
         _stream())


def rollout_mlp(env_id, W1, b1, W2, b2, Wm, bm, log_std, init, noise, states_rec, actions_rec,
                visited=None, maze=None):
    """All T steps of a batched MountainCar (env_id 0, init f64 [n,2]) / GridWorld (1, init f32) /
    box maze (2, init f32, with maze=) rollout with the 2-hidden-layer ReLU policy in one launch;
    noise [T, n, a] f64."""
    mz = _maze_arg("rollout_mlp", env_id, maze)
    _rollout_two_layer(env_id, mz, _lib.GOAL_NONE, W1, b1, W2.t().contiguous(), b2, Wm, bm,
                       log_std, init, noise, states_rec, actions_rec, visited=visited)


_NO_GOAL = (0.0, 0.0, 0, 0.0)  # (x, y, coord, value) of the entry points that take all four


def _rollout_mw(name, args, keep, ws, n, T, defer_check):
    """Calls the two-layer entry point `name` with its workspace and handles the error word, word
    0 (zeroed by the call): the multi-workgroup form gave up waiting for a part of a trajectory.
    The one-workgroup form (no workspace) sums in the same order and rewrites every output, so
    the result is the same bits either way: warn and re-run it (returns None), or with
    defer_check return (err, rerun) for the caller to do so.  `keep` holds the tensors behind
    `args` until the re-run."""
    call(name, *args, ptr(ws), ws.numel(), _stream())

    def rerun(_keep=keep):
        import warnings

        warnings.warn(f"{name}: workgroups of a trajectory were not co-resident; "
                      "re-ran the one-workgroup form")
        call(name, *args, None, 0, _stream())

    err = ws[:4].view(torch.int32)
    if defer_check:
        return err, rerun
    if n > 0 and T > 0 and int(err[0].item()) != 0:
        rerun()
    return None


def _rollout_two_layer(env_id, mz, kind, W1, b1, W2t, b2, Wm, bm, log_std, init, noise,
                       states_rec, actions_rec, visited=None, goal=_NO_GOAL,
                       goal_out=(None, None, None), defer_check=False):
    """The two-layer rollouts behind the wrappers' own checks: the C entry point of this
    (env_id, goal kind) -- mepol_rollout_maze with mz (env_id 2), else mepol_rollout_mlp,
    mepol_rollout_goal (ball) or mepol_rollout_goal_threshold -- its workspace and the error
    word (_rollout_mw).  goal = (x, y, coord, value), goal_out = (rewards_rec, len_out,
    done_out)."""
    T, n, a_dim = noise.shape
    h0, h1 = W1.shape[0], W2t.shape[1]
    if mz is not None and init.dtype != torch.float32:
        raise ValueError("a box maze's init is f32 [n, 2]")
    # (contiguous copies stay referenced until the launch is queued)
    W1, b1, b2, Wm, bm, log_std, init, noise = (t.contiguous() for t in (W1, b1, b2, Wm, bm,
                                                                          log_std, init, noise))
    gx, gy, coord, value = goal
    policy = (ptr(W1), ptr(b1), h0, ptr(W2t), ptr(b2), h1, ptr(Wm), ptr(bm), ptr(log_std), a_dim)
    init64, init32 = (ptr(init) if env_id == e else None for e in (0, 1))
    batch, recs = (ptr(noise), n, T), (ptr(states_rec), ptr(actions_rec))
    outs = tuple(ptr(t) for t in goal_out)
    if mz is not None:
        name, sizes = "mepol_rollout_maze", (kind, n, T, h0, h1, a_dim)
        args = (mz, kind, *policy, ptr(init), *batch, float(gx), float(gy), int(coord),
                float(value), *recs, ptr(visited), None, *outs)
    elif kind == _lib.GOAL_NONE:
        name, sizes = "mepol_rollout_mlp", (n, T, h0, h1, a_dim)
        args = (env_id, *policy, init64, init32, *batch, *recs, ptr(visited), None)
    elif kind == _lib.GOAL_BALL:
        name, sizes = "mepol_rollout_goal", (env_id, n, T, h0, h1, a_dim)
        args = (env_id, *policy, ptr(init), *batch, float(gx), float(gy), float(value), *recs,
                *outs)
    else:
        name, sizes = "mepol_rollout_goal_threshold", (env_id, n, T, h0, h1, a_dim)
        args = (env_id, *policy, init64, init32, *batch, int(coord), float(value), *recs, *outs)
    ws = _ws_or_cached(None, init.device, "rollout", name[len("mepol_"):], *sizes)
    return _rollout_mw(name, args, (W1, b1, W2t, b2, Wm, bm, log_std, init, noise), ws, n, T,
                       defer_check)


def _check_batch(who, noise, init, states_rec, actions_rec, visited, goal_out, policy_fits):
    """The shape check of the checked rollouts: `policy_fits` is the family's own half."""
    T, n, a_dim = noise.shape
    fits = (policy_fits and tuple(init.shape) == (n, 2) and tuple(states_rec.shape) == (n, T + 1, 2)
            and tuple(actions_rec.shape) == (n, T, a_dim)
            and (visited is None or tuple(visited.shape) == (n, T, 2)))
    if fits and goal_out is not None:
        rewards_rec, len_out, done_out = goal_out
        fits = tuple(rewards_rec.shape) == (n, T) and len_out.numel() == n and done_out.numel() == n
    if not fits:
        raise ValueError(f"{who}: tensor shapes do not fit the policy / batch")


def _check_dtypes(who, f64, f32, states_rec, actions_rec, visited=None, goal_out=None):
    """The dtype / contiguity check of the checked rollouts: `f64` and `f32` are the inputs of
    each type; the records are f32 (visited f64, len / done int32) and contiguous."""
    rewards = () if goal_out is None else goal_out[:1]
    ints = () if goal_out is None else goal_out[1:]
    vis = () if visited is None else (visited,)
    if (any(t.dtype != torch.float64 for t in (*f64, *vis))
            or any(t.dtype != torch.float32 for t in (*f32, states_rec, actions_rec, *rewards))
            or any(t.dtype != torch.int32 for t in ints)
            or not all(t.is_contiguous() for t in (states_rec, actions_rec, *vis, *rewards, *ints))):
        raise ValueError(f"{who}: f64 policy / noise / visited, f32 contiguous records"
                         if goal_out is None else
                         f"{who}: f64 policy / noise, f32 contiguous records, int32 len / done")


def _check_two_layer(who, W1, b1, W2, b2, Wm, bm, log_std, init, noise, states_rec, actions_rec,
                     goal_out, f32_init):
    """The two-layer goal rollouts' argument checks; f32_init: init must be f32 (else its dtype
    is the caller's to check)."""
    _require_device(init, noise, states_rec, actions_rec, *goal_out, W1, b1, W2, b2, Wm, bm,
                    log_std)
    a_dim, h0, h1 = noise.shape[2], W1.shape[0], W2.shape[0]
    _check_batch(who, noise, init, states_rec, actions_rec, None, goal_out,
                 tuple(W1.shape) == (h0, 2) and tuple(W2.shape) == (h1, h0)
                 and tuple(Wm.shape) == (a_dim, h1))
    _check_dtypes(who, (W1, b1, W2, b2, Wm, bm, log_std, noise), (init,) if f32_init else (),
                  states_rec, actions_rec, goal_out=goal_out)


def _check_deep(who, layers, Wm, bm, log_std, init, noise, states_rec, actions_rec, visited,
                goal_out, f64_init, f32_init):
    """The deep rollouts' argument checks; f64_init / f32_init: init must have that dtype (with
    neither, its dtype is the caller's to check)."""
    params = [t for p in layers for t in p]
    a_dim = noise.shape[2]
    fan_in = [2] + [W.shape[0] for W, _ in layers]
    _check_batch(who, noise, init, states_rec, actions_rec, visited, goal_out,
                 all(tuple(W.shape) == (b.numel(), f) for (W, b), f in zip(layers, fan_in))
                 and tuple(Wm.shape) == (a_dim, fan_in[-1]) and bm.numel() == a_dim
                 and log_std.numel() == a_dim)
    _check_dtypes(who, params + [Wm, bm, log_std, noise] + ([init] if f64_init else []),
                  (init,) if f32_init else (), states_rec, actions_rec, visited, goal_out)


def _rollout_deep_packed(env_id, mz, kind, layers, Wm, bm, log_std, init, noise, states_rec,
                         actions_rec, visited=None, goal=_NO_GOAL, goal_out=(None, None, None)):
    """The deep rollouts behind the wrappers' own checks: W_2 .. W_L transposed and packed, then
    the C entry point of this (env_id, goal kind) -- mepol_rollout_deep_maze with mz (env_id 2),
    else mepol_rollout_deep, mepol_rollout_deep_goal (ball) or mepol_rollout_deep_goal_threshold.
    goal = (x, y, coord, value), goal_out = (rewards_rec, len_out, done_out)."""
    T, n, a_dim = noise.shape
    (W1, b1), rest = layers[0], layers[1:]
    widths = (ctypes.c_int * len(layers))(*[W.shape[0] for W, _ in layers])
    Wt = torch.cat([W.t().reshape(-1) for W, _ in rest])
    bt = torch.cat([b.reshape(-1) for _, b in rest])
    # (contiguous copies stay referenced until the launch is queued)
    W1, b1, Wm, bm, log_std, init, noise = (t.contiguous() for t in (W1, b1, Wm, bm, log_std, init,
                                                                     noise))
    if mz is not None and init.dtype != torch.float32:
        raise ValueError("a box maze's init is f32 [n, 2]")
    gx, gy, coord, value = goal
    policy = (len(layers), widths, ptr(W1), ptr(b1), ptr(Wt), ptr(bt), ptr(Wm), ptr(bm),
              ptr(log_std), a_dim)
    init64, init32 = (ptr(init) if env_id == e else None for e in (0, 1))
    batch, recs = (ptr(noise), n, T), (ptr(states_rec), ptr(actions_rec))
    outs = tuple(ptr(t) for t in goal_out)
    if mz is not None:
        name = "mepol_rollout_deep_maze"
        args = (mz, kind, *policy, ptr(init), *batch, float(gx), float(gy), int(coord),
                float(value), *recs, ptr(visited), None, *outs)
    elif kind == _lib.GOAL_NONE:
        name = "mepol_rollout_deep"
        args = (env_id, *policy, init64, init32, *batch, *recs, ptr(visited), None)
    elif kind == _lib.GOAL_BALL:
        name = "mepol_rollout_deep_goal"
        args = (env_id, *policy, ptr(init), *batch, float(gx), float(gy), float(value), *recs,
                *outs)
    else:
        name = "mepol_rollout_deep_goal_threshold"
        args = (env_id, *policy, init64, init32, *batch, int(coord), float(value), *recs, *outs)
    # (the goal entry points share mepol_rollout_deep's workspace)
    ws = _ws_or_cached(None, init.device, "rollout",
                       "rollout_deep_maze" if mz is not None else "rollout_deep", n, T, len(layers),
                       widths, a_dim)
    call(name, *args, ptr(ws), ws.numel(), _stream())


def rollout_deep(env_id, layers, Wm, bm, log_std, init, noise, states_rec, actions_rec,
                 visited=None, maze=None):
    """rollout_mlp for a ReLU policy with 3 to 6 hidden layers, layers = [(W1, b1), ..., (W_L,
    b_L)] (widths <= 512, odd ones included): all T steps in one launch, one workgroup per
    trajectory (csrc/rollout_deep.hip).  W_2 .. W_L are transposed and packed here per call."""
    _require_device(init, noise, states_rec, actions_rec, visited, Wm, bm, log_std,
                    *[t for p in layers for t in p])
    mz = _maze_arg("rollout_deep", env_id, maze)
    _check_deep("rollout_deep", layers, Wm, bm, log_std, init, noise, states_rec, actions_rec,
                visited, None, env_id == 0, env_id != 0)
    _rollout_deep_packed(env_id, mz, _lib.GOAL_NONE, layers, Wm, bm, log_std, init, noise,
                         states_rec, actions_rec, visited=visited)


def _plan(name, *args):
    """{"workgroups_per_traj", "k_chunks"} of a two-layer *_plan_info entry point."""
    wg, kc = ctypes.c_int(), ctypes.c_int()
    call(name, *args, ctypes.byref(wg), ctypes.byref(kc))
    return {"workgroups_per_traj": wg.value, "k_chunks": kc.value}


def _deep_plan(name, widths, a_dim, *lead):
    """{"resident_workgroups"} of a deep *_plan_info entry point with its leading arguments."""
    wg = ctypes.c_int()
    arr = (ctypes.c_int * len(widths))(*[int(w) for w in widths])
    call(name, *lead, len(widths), arr, a_dim, ctypes.byref(wg))
    return {"resident_workgroups": wg.value}


def rollout_mlp_plan(n, h0, h1, a_dim, env_id=None):
    """{"workgroups_per_traj", "k_chunks"}: the form mepol_rollout_mlp takes for this shape and
    the layer-2 summation order it commits to (oracle.rollout_kordered's k_chunks).  env_id 2: the
    maze instance's own answer (MountainCar and GridWorld share one)."""
    if env_id == MAZE:
        return _plan("mepol_rollout_maze_plan_info", _lib.GOAL_NONE, n, h0, h1, a_dim)
    return _plan("mepol_rollout_mlp_plan_info", n, h0, h1, a_dim)


def rollout_deep_plan(env_id, widths, a_dim):
    """{"resident_workgroups"}: trajectories of rollout_deep itself (the instance without a goal
    on this env) the device holds at once for hidden layers of these widths."""
    if env_id == MAZE:
        return _deep_plan("mepol_rollout_deep_maze_plan_info", widths, a_dim, _lib.GOAL_NONE)
    return _deep_plan("mepol_rollout_deep_plan_info", widths, a_dim, env_id)


def rollout_goal_plan(n, h0, h1, a_dim=2, env_id=1):
    """rollout_mlp_plan for rollout_goal: the form the goal-mode kernel's own occupancy gives
    (env_id 2: the maze's ball-goal instance)."""
    if env_id == MAZE:
        return _plan("mepol_rollout_maze_plan_info", _lib.GOAL_BALL, n, h0, h1, a_dim)
    return _plan("mepol_rollout_goal_plan_info", n, h0, h1, a_dim)


def rollout_goal(W1, b1, W2, b2, Wm, bm, log_std, init, noise, goal_xy, radius, states_rec,
                 actions_rec, rewards_rec, len_out, done_out, env_id=1, defer_check=False,
                 maze=None):
    """rollout_mlp on GridWorld (env_id 1) or a box maze (env_id 2 with maze=) with early
    termination at a goal: a trajectory ends at
    the first step whose f32 state is within `radius` of goal_xy (reward 1, done), or after T
    steps.  Fills states_rec [n,T+1,2], actions_rec [n,T,2], rewards_rec [n,T] (f32, zeros behind
    each episode's end), len_out and done_out [n] int32; the buffers need no clearing.

    The error word is handled as rollout_mlp does: on a multi-workgroup refusal, warn and re-run
    the one-workgroup form (the same bits).  defer_check=True leaves that to the caller: the
    return value is (err, rerun), a device int32 [1] view of the word and the re-run, so the word
    can be read together with the caller's own results in one synchronisation."""
    goal_out = (rewards_rec, len_out, done_out)
    _check_two_layer("rollout_goal", W1, b1, W2, b2, Wm, bm, log_std, init, noise, states_rec,
                     actions_rec, goal_out, True)
    W2t = W2.t().contiguous()
    mz = _maze_arg("rollout_goal", env_id, maze)
    gx, gy = (float(v) for v in goal_xy)
    return _rollout_two_layer(env_id, mz, _lib.GOAL_BALL, W1, b1, W2t, b2, Wm, bm, log_std, init,
                              noise, states_rec, actions_rec, goal=(gx, gy, 0, radius),
                              goal_out=goal_out, defer_check=defer_check)


def rollout_deep_goal_plan(widths, a_dim=2, env_id=1):
    """{"resident_workgroups"}: trajectories of rollout_deep_goal the device holds at once for
    hidden layers of these widths (the goal-mode kernel's occupancy times the CU count; env_id 2:
    the maze's ball-goal instance)."""
    if env_id == MAZE:
        return _deep_plan("mepol_rollout_deep_maze_plan_info", widths, a_dim, _lib.GOAL_BALL)
    return _deep_plan("mepol_rollout_deep_goal_plan_info", widths, a_dim)


def rollout_deep_goal(layers, Wm, bm, log_std, init, noise, goal_xy, radius, states_rec,
                      actions_rec, rewards_rec, len_out, done_out, env_id=1, maze=None):
    """rollout_goal for a ReLU policy with 3 to 6 hidden layers, layers = [(W1, b1), ..., (W_L,
    b_L)] as rollout_deep takes them: GridWorld (env_id 1) episodes that end at the first step
    whose f32 state is within `radius` of goal_xy (reward 1, done) or after T steps, in one launch
    with one workgroup per trajectory (csrc/rollout_deep.hip, GOAL instance).  Fills states_rec
    [n,T+1,2], actions_rec [n,T,2], rewards_rec [n,T] (f32, zeros behind each episode's end),
    len_out and done_out [n] int32; the buffers need no clearing.  There is no error word to
    check: the workgroups exchange nothing."""
    _require_device(init, noise, states_rec, actions_rec, rewards_rec, len_out, done_out, Wm, bm,
                    log_std, *[t for p in layers for t in p])
    goal_out = (rewards_rec, len_out, done_out)
    _check_deep("rollout_deep_goal", layers, Wm, bm, log_std, init, noise, states_rec, actions_rec,
                None, goal_out, False, True)
    gx, gy = (float(v) for v in goal_xy)
    mz = _maze_arg("rollout_deep_goal", env_id, maze)
    _rollout_deep_packed(env_id, mz, _lib.GOAL_BALL, layers, Wm, bm, log_std, init, noise,
                         states_rec, actions_rec, goal=(gx, gy, 0, radius), goal_out=goal_out)


def _threshold_init(who, env_id, init):
    """The init tensor's dtype rule of the threshold-goal rollouts: f64 for MountainCar (env_id
    0), f32 for GridWorld (1) and the box maze (2)."""
    if env_id not in (0, 1, MAZE):
        raise ValueError(f"{who}: env_id 0 (MountainCar), 1 (GridWorld) or 2 (box maze)")
    if init.dtype != (torch.float64 if env_id == 0 else torch.float32):
        raise ValueError(f"{who}: init is f64 for MountainCar (env_id 0), f32 for GridWorld (1) "
                         "and the box maze (2)")


def rollout_goal_threshold_plan(env_id, n, h0, h1, a_dim=None):
    """rollout_goal_plan for rollout_goal_threshold on this env: the form the occupancy of the
    instance that runs (env x threshold goal) gives.  a_dim defaults to the env's."""
    a_dim = (1 if env_id == 0 else 2) if a_dim is None else a_dim
    if env_id == MAZE:
        return _plan("mepol_rollout_maze_plan_info", _lib.GOAL_THRESHOLD, n, h0, h1, a_dim)
    return _plan("mepol_rollout_goal_threshold_plan_info", env_id, n, h0, h1, a_dim)


def rollout_goal_threshold(env_id, W1, b1, W2, b2, Wm, bm, log_std, init, noise, coord, threshold,
                           states_rec, actions_rec, rewards_rec, len_out, done_out,
                           defer_check=False, maze=None):
    """rollout_goal with a threshold goal, on MountainCar (env_id 0, init f64 [n,2], one action)
    or GridWorld (1, init f32, two actions): a trajectory ends at the first step whose state has
    state[coord] >= threshold, compared in f64 on the env's own state (reward 1, done), or after T
    steps.  coord is 0 or 1; the threshold may be +-inf, not NaN.  Outputs, the error word,
    defer_check and the re-run of the one-workgroup form as rollout_goal."""
    goal_out = (rewards_rec, len_out, done_out)
    _check_two_layer("rollout_goal_threshold", W1, b1, W2, b2, Wm, bm, log_std, init, noise,
                     states_rec, actions_rec, goal_out, False)
    W2t = W2.t().contiguous()
    mz = _maze_arg("rollout_goal_threshold", env_id, maze)
    _threshold_init("rollout_goal_threshold", env_id, init)
    return _rollout_two_layer(env_id, mz, _lib.GOAL_THRESHOLD, W1, b1, W2t, b2, Wm, bm, log_std,
                              init, noise, states_rec, actions_rec,
                              goal=(0.0, 0.0, coord, threshold), goal_out=goal_out,
                              defer_check=defer_check)


def rollout_deep_goal_threshold_plan(env_id, widths, a_dim=None):
    """rollout_deep_goal_plan for rollout_deep_goal_threshold on this env (the occupancy of the
    instance that runs times the CU count).  a_dim defaults to the env's."""
    a_dim = (1 if env_id == 0 else 2) if a_dim is None else a_dim
    if env_id == MAZE:
        return _deep_plan("mepol_rollout_deep_maze_plan_info", widths, a_dim, _lib.GOAL_THRESHOLD)
    return _deep_plan("mepol_rollout_deep_goal_threshold_plan_info", widths, a_dim, env_id)


def rollout_deep_goal_threshold(env_id, layers, Wm, bm, log_std, init, noise, coord, threshold,
                                states_rec, actions_rec, rewards_rec, len_out, done_out,
                                maze=None):
    """rollout_goal_threshold for a ReLU policy with 3 to 6 hidden layers, layers = [(W1, b1), ...,
    (W_L, b_L)] as rollout_deep takes them: one launch with one workgroup per trajectory
    (csrc/rollout_deep.hip, threshold instance), no error word to check."""
    _require_device(init, noise, states_rec, actions_rec, rewards_rec, len_out, done_out, Wm, bm,
                    log_std, *[t for p in layers for t in p])
    goal_out = (rewards_rec, len_out, done_out)
    _check_deep("rollout_deep_goal_threshold", layers, Wm, bm, log_std, init, noise, states_rec,
                actions_rec, None, goal_out, False, False)
    _threshold_init("rollout_deep_goal_threshold", env_id, init)
    mz = _maze_arg("rollout_deep_goal_threshold", env_id, maze)
    _rollout_deep_packed(env_id, mz, _lib.GOAL_THRESHOLD, layers, Wm, bm, log_std, init, noise,
                         states_rec, actions_rec, goal=(0.0, 0.0, coord, threshold),
                         goal_out=goal_out)


def traj_budget(lens, dones, budget):
    """The step budget over a parallel batch (mepol_traj_budget): trajectories in index order until
    `budget` steps are kept, the last one cut.  lens, dones: int32 [n] on the device.  Returns
    (len_out int32 [n], done_out int32 [n], offsets int64 [n+1], meta int64 [2] = {trajectories
    used, steps kept}), all on the device."""
    _require_device(lens, dones)
    n = lens.numel()
    if lens.dtype != torch.int32 or dones.dtype != torch.int32 or dones.numel() != n:
        raise ValueError("traj_budget: int32 lens and dones of one size")
    dev = lens.device
    len_out = torch.empty(n, dtype=torch.int32, device=dev)
    done_out = torch.empty(n, dtype=torch.int32, device=dev)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    meta = torch.zeros(2, dtype=torch.int64, device=dev)
    call("mepol_traj_budget", ptr(lens.contiguous()), ptr(dones.contiguous()), n, int(budget),
         ptr(len_out), ptr(done_out), ptr(offsets), ptr(meta), _stream())
    return len_out, done_out, offsets, meta


def traj_cut(done_step, rewards, states_rec, actions_rec):
    """The episodes inside un-terminated rollouts (mepol_traj_cut): every trajectory is cut at its
    first step t with done_step[i, t] set, IN PLACE.  done_step [n,T] bool or uint8 (any non-zero
    byte), rewards [n,T] f32, states_rec [n,T+1,nf] f32, actions_rec [n,T,a] f32, all contiguous on
    the device: rewards[i, len:], actions_rec[i, len:] and states_rec[i, len + 1:] become +0.0,
    everything before keeps its bits.  Returns (lens int32 [n], dones int32 [n]): len = t + 1 and
    done = 1 at a first hit, else len = T and done = 0 -- what the goal rollouts write."""
    _require_device(done_step, rewards, states_rec, actions_rec)
    if rewards.dim() != 2 or states_rec.dim() != 3 or actions_rec.dim() != 3:
        raise ValueError("traj_cut: rewards [n,T], states_rec [n,T+1,nf], actions_rec [n,T,a]")
    n, T = rewards.shape
    nf, a = states_rec.shape[2], actions_rec.shape[2]
    if (tuple(done_step.shape) != (n, T) or tuple(states_rec.shape) != (n, T + 1, nf)
            or tuple(actions_rec.shape) != (n, T, a)):
        raise ValueError("traj_cut: tensor shapes do not fit the batch")
    if (done_step.dtype not in (torch.bool, torch.uint8) or rewards.dtype != torch.float32
            or states_rec.dtype != torch.float32 or actions_rec.dtype != torch.float32):
        raise ValueError("traj_cut: bool or uint8 done_step, f32 rewards / records")
    if not all(t.is_contiguous() for t in (done_step, rewards, states_rec, actions_rec)):
        raise ValueError("traj_cut: contiguous tensors are needed (the records are cut in place)")
    if len({t.device for t in (done_step, rewards, states_rec, actions_rec)}) != 1:
        raise ValueError("traj_cut: tensors on one device")
    dev = rewards.device
    lens = torch.empty(n, dtype=torch.int32, device=dev)
    dones = torch.empty(n, dtype=torch.int32, device=dev)
    call("mepol_traj_cut", ptr(done_step), n, T, ptr(rewards), ptr(states_rec), nf,
         ptr(actions_rec), a, ptr(lens), ptr(dones), _stream())
    return lens, dones


def gae(rewards, values, lens, dones, offsets, n_out, gamma, lambd, states_rec, actions_rec):
    """Targets, GAE advantages and the packed batch of ragged trajectories (mepol_gae).  rewards
    [n,T] f32, values [n,T+1] f64, lens / dones int32 [n], offsets int64 [n+1] (traj_budget's),
    n_out = offsets[n] (a host int), states_rec [n,T+1,nf] and actions_rec [n,T,a] f32.  Returns
    (targets [n_out], adv [n_out], states [n_out,nf], actions [n_out,a]), all f64."""
    _require_device(rewards, values, lens, dones, offsets, states_rec, actions_rec)
    n, T = rewards.shape
    nf, a = states_rec.shape[2], actions_rec.shape[2]
    if (tuple(values.shape) != (n, T + 1) or tuple(states_rec.shape) != (n, T + 1, nf)
            or tuple(actions_rec.shape) != (n, T, a) or lens.numel() != n or dones.numel() != n
            or offsets.numel() != n + 1):
        raise ValueError("gae: tensor shapes do not fit the batch")
    if (rewards.dtype != torch.float32 or values.dtype != torch.float64
            or states_rec.dtype != torch.float32 or actions_rec.dtype != torch.float32
            or lens.dtype != torch.int32 or dones.dtype != torch.int32
            or offsets.dtype != torch.int64):
        raise ValueError("gae: f32 rewards / records, f64 values, int32 lens / dones, int64 offsets")
    rewards, values, lens, dones, offsets, states_rec, actions_rec = (
        t.contiguous() for t in (rewards, values, lens, dones, offsets, states_rec, actions_rec))
    dev = rewards.device
    n_out = int(n_out)
    f64 = dict(dtype=torch.float64, device=dev)
    targets, adv = torch.empty(n_out, **f64), torch.empty(n_out, **f64)
    states, actions = torch.empty((n_out, nf), **f64), torch.empty((n_out, a), **f64)
    call("mepol_gae", ptr(rewards), ptr(values), ptr(lens), ptr(dones), ptr(offsets), n, T, n_out,
         float(gamma), float(lambd), ptr(states_rec), nf, ptr(actions_rec), a, ptr(targets),
         ptr(adv), ptr(states), ptr(actions), _stream())
    return targets, adv, states, actions


def standardize(x, out=None):
    """(x - mean) / population std of an f64 vector on the device (mepol_standardize): the same
    bits on every call; a zero std gives non-finite values, as numpy does."""
    _require_device(x, out)
    if x.dim() != 1 or x.dtype != torch.float64 or not x.is_contiguous():
        raise ValueError("standardize: a contiguous f64 vector is needed")
    n = x.numel()
    res = out if out is not None else torch.empty_like(x)
    assert res.shape == x.shape and res.dtype == x.dtype and res.is_contiguous()
    ws = _ws_or_cached(None, x.device, "standardize", "standardize", n)
    call("mepol_standardize", ptr(x), n, ptr(res), ptr(ws), ws.numel(), _stream())
    return res


def memcpy_async(dst, src):
    """dst <- src (same byte size; device or pinned host tensors), ordered on the current
    stream; inside a graph capture this is a memcpy node."""
    nbytes = src.numel() * src.element_size()
    assert dst.numel() * dst.element_size() == nbytes and dst.is_contiguous() and src.is_contiguous()
    call("mepol_memcpy_async", ptr(dst), ptr(src), nbytes, _stream())


def volume_constant(ns, G):
    return math.pi ** (ns / 2) / G
