"""Thin tensor-level wrappers over the C ABI (one Python function per entry point of include/cogview_hip.h).

torch is used for device memory, streams and shapes only; every FLOP / byte of the hot path happens inside
libcogview_hip.so.  All functions require CUDA(HIP) tensors and raise otherwise -- there is no CPU path.
"""
import ctypes as C
import os

import torch

from . import _lib as L

_DT = {torch.float16: L.F16, torch.bfloat16: L.BF16, torch.float32: L.F32}


def dt_code(t):
    try:
        return _DT[t.dtype if isinstance(t, torch.Tensor) else t]
    except KeyError:
        raise L.CogviewHipError(f"unsupported dtype {t.dtype if isinstance(t, torch.Tensor) else t}")


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.CogviewHipError(
                "cogview_amd ops run only on an MI355X (HIP) device: got a CPU tensor and there is no CPU fallback")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------ scratch
_WS = {}


def workspace(tag, nbytes, device, floor=1 << 20):
    """Stream-ordered scratch (one buffer per tag and device, grown geometrically; `floor`: smallest allocation -- 0 for the
    small per-stream tags)."""
    key = (tag, device.index if device.index is not None else torch.cuda.current_device())
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes * 1.25), int(floor), 256), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


class _ScalarPool:
    """Zero-initialised fp32 device scalars (abs-max slots for Sandwich-LN).  Slots are never recycled:
    a fresh zeroed slab (one memset) is allocated every `n` requests and kept alive by its views."""

    def __init__(self, n=2048):
        self.n, self.slab, self.i = n, {}, {}

    def next(self, device):
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self.slab or self.i[key] >= self.n:
            self.slab[key] = torch.zeros(self.n, dtype=torch.float32, device=device)
            self.i[key] = 0
        s = self.slab[key][self.i[key]:self.i[key] + 1]
        self.i[key] += 1
        return s


_scalars = _ScalarPool()


class scalar_slab:
    """Context manager: abs-max slots come, in order, from the caller's zeroed fp32 slab instead of the pool.  A captured
    decode step (generation/decoder.py) needs slots at FIXED addresses that its own first node clears on every replay."""

    def __init__(self, slab):
        self.slab, self.i = slab, 0

    def next(self, device):
        assert self.i < self.slab.numel(), "scalar slab exhausted"
        s = self.slab[self.i:self.i + 1]
        self.i += 1
        return s

    def __enter__(self):
        global _scalars
        self.saved, _scalars = _scalars, self
        self.i = 0
        return self

    def __exit__(self, *exc):
        global _scalars
        _scalars = self.saved
        return False


def new_absmax_slot(device):
    return _scalars.next(device)


# ------------------------------------------------------------------------------------------ GEMM
_GEMM_TIMING = None      # list of (variant, flops, start_event, end_event) while bench.py's timed region runs


def enable_gemm_timing():
    """Bracket every cogv_gemm launch with HIP events on the launch stream (bench.py's roofline leg)."""
    global _GEMM_TIMING
    _GEMM_TIMING = []
    return _GEMM_TIMING


_GEMM_TIMING_PARKED = None


def sample_gemm_timing(active):
    """Inside the timed region: bracket the launches of THIS step (active) or let it run bare.  bench.py samples one step
    in four -- 870 event records per sampled 4B step cost 0.6 % of the step when every step carries them
    (profiles/r04_bench_event_overhead_ab.log)."""
    global _GEMM_TIMING, _GEMM_TIMING_PARKED
    if active and _GEMM_TIMING is None and _GEMM_TIMING_PARKED is not None:
        _GEMM_TIMING, _GEMM_TIMING_PARKED = _GEMM_TIMING_PARKED, None
    elif not active and _GEMM_TIMING is not None:
        _GEMM_TIMING_PARKED, _GEMM_TIMING = _GEMM_TIMING, None


def collect_gemm_timing():
    """Synchronise, resolve the events and return aggregate statistics; disables timing."""
    global _GEMM_TIMING, _GEMM_TIMING_PARKED
    if _GEMM_TIMING is None:
        _GEMM_TIMING, _GEMM_TIMING_PARKED = _GEMM_TIMING_PARKED, None
    rec, _GEMM_TIMING = _GEMM_TIMING, None
    torch.cuda.synchronize()
    tot_ms, tot_fl, tot_by, by, shapes = 0.0, 0.0, 0.0, {}, {}
    for rec_i in rec:
        variant, fl, nbytes, s, e = rec_i[:5]
        ms = s.elapsed_time(e)
        tot_ms += ms
        tot_fl += fl
        tot_by += nbytes
        a = by.setdefault(variant, [0.0, 0.0, 0, 0.0])
        a[0] += fl
        a[1] += ms
        a[2] += 1
        a[3] += nbytes
        if len(rec_i) > 5:
            a = shapes.setdefault(f"{variant} {rec_i[5]}", [0.0, 0.0, 0, 0.0])
            a[0] += fl
            a[1] += ms
            a[2] += 1
            a[3] += nbytes
    n = max(len(rec), 1)

    def agg(keys):
        """totals over the kernel families `keys` (the GEMM roofline counts GEMM launches only)"""
        fl, ms, cnt, nb = (sum(by[k][i] for k in keys if k in by) for i in range(4))
        return {"launches": cnt, "total_ms": ms, "avg_ms": ms / max(cnt, 1), "algo_bytes": nb, "tflops": fl / max(ms, 1e-9) / 1e9}

    def entry(v):
        return {"tflops": v[0] / max(v[1], 1e-9) / 1e9, "launches": v[2], "avg_ms": v[1] / v[2], "total_ms": v[1],
                "algo_gbytes_per_s": v[3] / max(v[1], 1e-9) / 1e6}

    out = agg(list(by))
    out.update({"by_variant": {k: entry(v) for k, v in by.items()},
                "by_shape": {k: {"tflops": round(v[0] / max(v[1], 1e-9) / 1e9, 1), "launches": v[2], "avg_ms": round(v[1] / v[2], 4),
                                 "gbytes_per_s": round(v[3] / max(v[1], 1e-9) / 1e6, 1)}
                             for k, v in sorted(shapes.items(), key=lambda kv: -kv[1][1])},
                "gemm": agg(GEMM_FAMILIES)})
    return out


GEMM_FAMILIES = ("NT_fwd", "NN_dgrad", "TN_wgrad", "TN_other")


class timed_launch:
    """Bracket a launch of any other kernel family with HIP events on the launch stream while bench.py's timed region
    runs (same record list as the GEMMs): `with timed_launch("conv", flops, bytes, "label"): <launch>`."""
    __slots__ = ("rec",)

    def __init__(self, family, flops, nbytes, label):
        # flops / label may be callables: they are only evaluated while a timed region runs (~1500 launches per 4B step build
        # their label strings for nothing otherwise)
        self.rec = None
        if _GEMM_TIMING is not None:
            self.rec = [family, float(flops() if callable(flops) else flops), float(nbytes), torch.cuda.Event(enable_timing=True),
                        torch.cuda.Event(enable_timing=True), label() if callable(label) else label]

    def __enter__(self):
        if self.rec is not None:
            self.rec[3].record()
        return self

    def __exit__(self, *exc):
        if self.rec is not None and _GEMM_TIMING is not None:
            self.rec[4].record()
            _GEMM_TIMING.append(tuple(self.rec))
        return False


def gemm(a, b, trans_a=False, trans_b=False, out=None, bias=None, gelu=False, gelu_aux=None, dgelu_aux=None,
         dropout=None, absmax=None, accumulate=False, splitk=None, out_dtype=None, variant=0, colsum_out=None,
         colsum_accumulate=True, gelu_daux=None, mul_aux=None, dropout_row0=0):
    """C[M,N] = epilogue(A_op[M,K] . B_op[N,K]^T); a, b 2-D, last dim contiguous.
    trans_a: `a` is stored [K, M];  trans_b: `b` is stored [K, N].
    gelu_aux [M,N]: receives the rounded pre-activation; gelu_daux [M,N] (instead): receives gelu'(pre-activation), which
    the backward GEMM applies with mul_aux (out = x * mul_aux) -- one multiply where dgelu_aux re-evaluates the sigmoid.
    dropout = (p, seed, stream_id); dropout_row0: the call computes rows [row0, row0 + M) of a larger tensor whose mask it
    draws (row chunks of a row-parallel Linear).  colsum_out [N]: (+)= column sums of C (the bias gradient of the layer whose
    output gradient C is), fused into the epilogue when the shape allows, otherwise a separate pass.  Returns C."""
    _need_gpu(a, b)
    assert a.dim() == 2 and b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1
    if trans_a:
        K, M = a.shape
    else:
        M, K = a.shape
    if trans_b:
        Kb, N = b.shape
    else:
        N, Kb = b.shape
    assert K == Kb, f"contraction mismatch {K} vs {Kb}"
    d = L.GemmDesc()
    d.dtype = dt_code(a)
    d.trans_a, d.trans_b = int(trans_a), int(trans_b)
    d.M, d.N, d.K = M, N, K
    d.A, d.lda = a.data_ptr(), a.stride(0)
    d.B, d.ldb = b.data_ptr(), b.stride(0)
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype or a.dtype, device=a.device)
        assert not accumulate
    assert out.shape == (M, N) and out.stride(1) == 1
    d.C, d.ldc = out.data_ptr(), out.stride(0)
    d.out_f32 = int(out.dtype == torch.float32)
    flags = 0
    if bias is not None:
        flags |= L.EPI_BIAS
        d.bias = bias.data_ptr()
    if gelu:
        flags |= L.EPI_GELU
        assert gelu_aux is None or gelu_daux is None
        if gelu_aux is not None:
            d.aux, d.ldaux = gelu_aux.data_ptr(), gelu_aux.stride(0)
        if gelu_daux is not None:
            flags |= L.EPI_GELU_DAUX
            d.aux, d.ldaux = gelu_daux.data_ptr(), gelu_daux.stride(0)
    if dgelu_aux is not None:
        flags |= L.EPI_DGELU
        d.aux, d.ldaux = dgelu_aux.data_ptr(), dgelu_aux.stride(0)
    if mul_aux is not None:
        assert dgelu_aux is None and not gelu
        flags |= L.EPI_MULAUX
        d.aux, d.ldaux = mul_aux.data_ptr(), mul_aux.stride(0)
    if dropout is not None and dropout[0] > 0.0:
        flags |= L.EPI_DROPOUT
        d.dropout_p, d.seed, d.stream_id = float(dropout[0]), int(dropout[1]), int(dropout[2])
        d.dropout_row0 = int(dropout_row0)
    if absmax is not None:
        flags |= L.EPI_ABSMAX
        d.absmax = absmax.data_ptr()
    if accumulate:
        flags |= L.EPI_ACCUM
    lib = L.lib()
    fuse_colsum = colsum_out is not None and _fuse_colsum(d, variant)
    if fuse_colsum:
        flags |= L.EPI_COLSUM
        cs_rows = lib.cogv_gemm_colsum_rows(M)
        cs_ws = workspace("gemm_colsum", cs_rows * N * 4, a.device)
        d.colsum_partial = cs_ws.data_ptr()
        splitk = 1
    d.flags = flags
    if splitk is None:
        splitk = lib.cogv_gemm_pick_splitk(M, N, K)
    d.splitk = int(splitk)
    d.kernel_variant = int(variant)
    if d.splitk > 1:
        nbytes = lib.cogv_gemm_workspace_bytes(C.byref(d))
        ws = workspace("gemm_splitk", nbytes, a.device)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    if _GEMM_TIMING is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        L.check(lib.cogv_gemm(C.byref(d), _stream()), "cogv_gemm")
        ev1.record()
        variant = ("T" if trans_a else "N") + ("T" if trans_b else "N")
        _GEMM_TIMING.append(({"NN": "NT_fwd", "NT": "NN_dgrad", "TT": "TN_wgrad", "TN": "TN_other"}[variant],
                             2.0 * M * N * K, 2.0 * (M * K + N * K + M * N), ev0, ev1, f"{M}x{N}x{K} epi={flags}"))
    else:
        L.check(lib.cogv_gemm(C.byref(d), _stream()), "cogv_gemm")
    if colsum_out is not None:
        if fuse_colsum:
            L.check(lib.cogv_colsum_finalize(dt_code(out), d.colsum_partial, cs_rows, N, _p(colsum_out), int(colsum_accumulate),
                                             _stream()), "cogv_colsum_finalize")
        else:
            colsum(out, out=colsum_out, accumulate=colsum_accumulate)
    return out


def _persistent_takes(d, colsum=False):
    """The library's answer (cogv_gemm_plan, host only) to: does the persistent kernel -- generation 4, the one that fuses the
    column sums and the one cogv_gemm_grouped launches -- take the problem of descriptor d?  Asked with kernel_variant 10, which
    falls back to auto dispatch where it does not; with `colsum`, asked as the COGV_EPI_COLSUM launch itself (no split-K; the
    partial-sum pointer is an aligned stand-in that nothing reads)."""
    q = L.GemmDesc.from_buffer_copy(d)
    q.kernel_variant, q.splitk, q.flags, q.colsum_partial = 10, 1, L.EPI_COLSUM if colsum else 0, 16
    rc, plan = L.gemm_plan(q)
    return rc == L.OK and plan[0]["family"] == 0 and plan[0]["generation"] == 4


def _fuse_colsum(d, variant):
    """gemm's policy for the bias gradient: fused into the epilogue of a 16-bit, auto-dispatched (or generation 3 / 4) product
    whose A is stored [M, K], where the library takes it; a separate pass over the output otherwise."""
    return not d.trans_a and variant in (0, 9, 10) and not d.out_f32 and _persistent_takes(d, colsum=True)


def gemm_reserve_cus(n):
    """The persistent GEMM launches leave `n` CUs free from now on (cogv_gemm_reserve_cus; room for a concurrent collective's
    channel workgroups); returns the previous setting."""
    return int(L.lib().cogv_gemm_reserve_cus(int(n)))


def _skinny_desc(out, K, bias, gelu, absmax):
    """The descriptor of a skinny-M product into out [M, N] with its epilogue flags; the operands (A, B / ldb or an 8-bit
    weight) are the caller's."""
    d = L.GemmDesc()
    d.dtype = dt_code(out)
    d.M, d.N, d.K = out.shape[0], out.shape[1], K
    d.A, d.lda = None, K
    d.C, d.ldc = out.data_ptr(), out.shape[1]
    flags = 0
    if bias is not None:
        flags |= L.EPI_BIAS
        d.bias = bias.data_ptr()
    if gelu:
        flags |= L.EPI_GELU
    if absmax is not None:
        flags |= L.EPI_ABSMAX
        d.absmax = absmax.data_ptr()
    d.flags, d.splitk = flags, 1
    return d


def gemm_rows(a, w, bias=None, gelu=False, absmax=None, out=None):
    """The wide product of a decode step (cogv_gemm_rows): out [M, N] = epilogue(a [M, K] . w [N, K]^T + bias) for 1 <= M <= 64
    rows on a 16-bit weight, streamed once like gemm's skinny case (N % 8 == 0, 512 <= K <= 10240, K % 512 == 0).  Rows of a, w
    and a given `out` may be strided.  Shapes outside raise: there is no other kernel behind this one."""
    _need_gpu(a, w)
    assert a.dim() == 2 and w.dim() == 2 and a.stride(1) == 1 and w.stride(1) == 1 and a.dtype == w.dtype
    M, K = a.shape
    N, Kw = w.shape
    assert K == Kw, f"contraction mismatch {K} vs {Kw}"
    assert bias is None or bias.dtype == a.dtype
    if out is None:
        out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    assert out.shape == (M, N) and out.dtype == a.dtype and out.stride(1) == 1
    d = _skinny_desc(out, K, bias, gelu, absmax)
    d.ldc = out.stride(0)
    d.A, d.lda = a.data_ptr(), a.stride(0)
    d.B, d.ldb = w.data_ptr(), w.stride(0)
    L.check(L.lib().cogv_gemm_rows(C.byref(d), _stream()), "cogv_gemm_rows")
    return out


_Q_SUFFIX = {"e4m3": "_w8", "mxfp4": "_w4"}       # weight format -> what the C entry points of its products end in


def _q_operand(fmt, qs, K=None):
    """(N, K, cogv_w8_weight | cogv_w4_weight) of the quantized weight qs = (q, scale) of format `fmt`, validated.  K: the
    contraction length the product's input has (None: the weight's own)."""
    q, scale = qs
    _need_gpu(q, scale)
    per_byte, what = (2, "q [N, K / 2] uint8") if fmt == "mxfp4" else (1, "q [N, K] uint8")
    assert q.dim() == 2 and q.dtype == torch.uint8 and q.stride(1) == 1 and K in (None, q.shape[1] * per_byte), \
        what + ("" if K is None else " with K matching the input")
    N, K = q.shape[0], q.shape[1] * per_byte
    if fmt == "mxfp4":
        assert scale.dim() == 2 and scale.dtype == torch.uint8 and scale.stride(1) == 1 and scale.shape == (N, K // 32)
        w = L.W4Weight()
        w.lds = scale.stride(0)
    else:
        assert scale.dtype == torch.float32 and scale.is_contiguous() and scale.numel() == N
        w = L.W8Weight()
    w.q, w.ldq, w.scale = q.data_ptr(), q.stride(0), scale.data_ptr()
    return N, K, w


def _gemm_rows_q(fmt, a, qs, bias, gelu, absmax, out):
    N, K, w = _q_operand(fmt, qs)
    _need_gpu(a)
    assert a.dim() == 2 and a.stride(1) == 1 and a.shape[1] == K, "a [M, K] with K matching the weight"
    assert bias is None or bias.dtype == a.dtype
    M = a.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    assert out.shape == (M, N) and out.dtype == a.dtype and out.stride(1) == 1
    d = _skinny_desc(out, K, bias, gelu, absmax)
    d.ldc = out.stride(0)
    d.A, d.lda = a.data_ptr(), a.stride(0)
    name = "cogv_gemm_rows" + _Q_SUFFIX[fmt]
    L.check(getattr(L.lib(), name)(C.byref(d), C.byref(w), _stream()), name)
    return out


def gemm_rows_w8(a, qs, bias=None, gelu=False, absmax=None, out=None):
    """gemm_rows on an 8-bit weight qs = (q [N, K] uint8, scale [N] fp32) from quantize_rows_e4m3 (cogv_gemm_rows_w8): out [M, N] =
    epilogue(scale * (a . e4m3(q)^T) + bias) in a's dtype for 1 <= M <= 64 rows; gemm_w8 stops at 8.  Rows of a, q and a given
    `out` may be strided (q: a multiple of 16 bytes).  Shapes outside raise: there is no other kernel."""
    return _gemm_rows_q("e4m3", a, qs, bias, gelu, absmax, out)


def gemm_rows_w4(a, qs, bias=None, gelu=False, absmax=None, out=None):
    """gemm_rows on a 4-bit weight qs = (q [N, K / 2] uint8, scale [N, K / 32] uint8) from quantize_rows_mxfp4 (cogv_gemm_rows_w4):
    out [M, N] = epilogue(a . dequantize_rows_mxfp4(q, scale)^T + bias) in a's dtype for 1 <= M <= 64 rows; gemm_w4 stops at 8.
    Rows of a, q (a multiple of 16 bytes), scale and a given `out` may be strided.  Shapes outside raise: there is no other kernel."""
    return _gemm_rows_q("mxfp4", a, qs, bias, gelu, absmax, out)


def _ln_prologue(z, gamma, beta, eps, z_absmax, post, residual, want_t):
    """(cogv_ln_prologue, t [M, K] or None) of gemv_ln / gemv_ln_w8; z and (post-LN form) gamma share the product's 16-bit type."""
    # fp32 residual stream (see sandwich_ln_fwd): the residual of the post-LN form, or z itself in the plain-input form
    stream32 = (residual.dtype == torch.float32) if post is not None else (z.dtype == torch.float32)
    ln = L.LnPrologue()
    ln.z = z.data_ptr()
    ln.z_absmax = None if z_absmax is None else z_absmax.data_ptr()
    t = None
    if post is not None:
        assert z.dtype == gamma.dtype
        assert residual is not None and residual.is_contiguous() and residual.shape == z.shape     # z_absmax None: taken in the kernel
        ln.gamma_post, ln.beta_post, ln.residual = post[0].data_ptr(), post[1].data_ptr(), residual.data_ptr()
        if want_t:
            t = torch.empty_like(residual)
            ln.t_out = t.data_ptr()
    ln.gamma, ln.beta, ln.eps = gamma.data_ptr(), beta.data_ptr(), float(eps)
    ln.stream_f32 = int(stream32)
    return ln, t


def gemv_ln(z, w, bias, gamma, beta, eps, z_absmax=None, post=None, residual=None, want_t=False, gelu=False, absmax=None):
    """Decode-step GEMV with its LayerNorms as prologue (cogv_gemv_ln): z [M, K] (M <= 8), w [N, K].
        t = residual + SandwichLN(z; post = (gamma_p, beta_p), scale z_absmax)   (post given)   else   t = z
        out = epilogue(SandwichLN(t; gamma, beta) . w^T + bias)
    Returns (out [M, N], t [M, K] or None)."""
    _need_gpu(z, w)
    assert z.dim() == 2 and w.dim() == 2 and z.is_contiguous() and w.stride(1) == 1 and z.shape[1] == w.shape[1]
    assert post is None or z.dtype == w.dtype
    M, K = z.shape
    out = torch.empty((M, w.shape[0]), dtype=w.dtype, device=z.device)
    d = _skinny_desc(out, K, bias, gelu, absmax)
    d.A = z.data_ptr()
    d.B, d.ldb = w.data_ptr(), w.stride(0)
    ln, t = _ln_prologue(z, gamma, beta, eps, z_absmax, post, residual, want_t)
    L.check(L.lib().cogv_gemv_ln(C.byref(d), C.byref(ln), _stream()), "cogv_gemv_ln")
    return out, t


def gemm_grouped(problems, trans_a=True, trans_b=True, accumulate=True):
    """Up to 16 GEMMs of one layout in ONE persistent launch (cogv_gemm_grouped): `problems` is a list of
    (a, b, out) or (a, b, out, accumulate) -- the flag is per problem, `accumulate` its default.  Used for the weight gradients of one or several transformer layers, which fill the 256 CUs together.
    Falls back to one cogv_gemm per problem when the library reports a shape the grouped kernel does not take."""
    assert 1 <= len(problems) <= 16
    lib = L.lib()
    descs = (L.GemmDesc * len(problems))()
    tiles, kmin, flops, nbytes = 0, None, 0.0, 0.0
    shapes = []
    problems = [(pr[0], pr[1], pr[2], pr[3] if len(pr) > 3 else accumulate) for pr in problems]
    for d, (a, b, out, acc) in zip(descs, problems):
        _need_gpu(a, b, out)
        assert a.dim() == 2 and b.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1 and out.stride(1) == 1
        K, M = a.shape if trans_a else a.shape[::-1]
        Kb, N = b.shape if trans_b else b.shape[::-1]
        assert K == Kb and out.shape == (M, N)
        d.dtype = dt_code(a)
        d.trans_a, d.trans_b = int(trans_a), int(trans_b)
        d.M, d.N, d.K = M, N, K
        d.A, d.lda = a.data_ptr(), a.stride(0)
        d.B, d.ldb = b.data_ptr(), b.stride(0)
        d.C, d.ldc = out.data_ptr(), out.stride(0)
        d.out_f32 = int(out.dtype == torch.float32)
        d.flags = L.EPI_ACCUM if acc else 0
        shapes.append((M, N, K))
        tiles += ((M + 255) // 256) * ((N + 255) // 256)
        kmin = K if kmin is None else min(kmin, K)
        flops += 2.0 * M * N * K
        nbytes += 2.0 * (M * K + N * K + M * N)
    if not all(_persistent_takes(d) for d in descs):
        for a, b, out, acc in problems:
            gemm(a, b, trans_a=trans_a, trans_b=trans_b, out=out, accumulate=acc)
        return
    splitk = lib.cogv_gemm_pick_splitk_tiles(tiles, kmin)
    if splitk > 1:
        sizes = [splitk * M * N * 4 for M, N, _ in shapes]
        ws = workspace("gemm_grouped_splitk", sum(sizes), problems[0][0].device)
        off = 0
        for d, sz in zip(descs, sizes):
            d.splitk, d.workspace, d.workspace_bytes = splitk, ws.data_ptr() + off, sz
            off += sz
    else:
        for d in descs:
            d.splitk = 1
    if _GEMM_TIMING is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        L.check(lib.cogv_gemm_grouped(descs, len(problems), _stream()), "cogv_gemm_grouped")
        ev1.record()
        key = {(False, False): "NT_fwd", (False, True): "NN_dgrad", (True, True): "TN_wgrad"}.get((trans_a, trans_b), "TN_other")
        _GEMM_TIMING.append((key, flops, nbytes, ev0, ev1, f"grouped, {tiles} tiles of 256x256 ({tiles / 256:.2f} rounds), K={kmin}"))
    else:
        L.check(lib.cogv_gemm_grouped(descs, len(problems), _stream()), "cogv_gemm_grouped")


# ------------------------------------------------------------------------------------------ Sandwich-LN
LN_ALL_T, LN_STREAM_IN, LN_STREAM_OUT = 0, 1, 2       # cogview_hip.h COGV_LN_*
_LN_MODE_NAME = {0: "16-bit", 1: "stream in (fp32 -> 16-bit)", 2: "stream out (16-bit + fp32 -> fp32)"}


def sandwich_ln_fwd(x, gamma, beta, eps, absmax_in, residual=None, absmax_out=None, save_stats=True):
    """y = [residual +] SandwichLN(x).  The fp32 RESIDUAL STREAM is recognised by dtype: an fp32 `x` (with 16-bit
    gamma) is the stream feeding a branch -> y in gamma's type (LN1, LN2, final LN); an fp32 `residual` is the stream
    a branch output joins -> y fp32 = residual + LN(x), no rounding in between (LN3, LN4)."""
    _need_gpu(x, gamma, beta)
    h = x.shape[-1]
    x2 = x.reshape(-1, h)
    assert x2.is_contiguous()
    rows = x2.shape[0]
    mode, ydt = LN_ALL_T, gamma.dtype
    r2 = None
    if residual is not None:
        r2 = residual.reshape(-1, h)
        assert r2.is_contiguous()
        if residual.dtype == torch.float32:
            mode, ydt = LN_STREAM_OUT, torch.float32
        elif residual.dtype != gamma.dtype:
            raise L.CogviewHipError("Sandwich-LN residual must be fp32 (the residual stream) or the storage type")
    if x.dtype == torch.float32:
        if mode == LN_STREAM_OUT:
            raise L.CogviewHipError("Sandwich-LN: an fp32 input with an fp32 residual is not a form the layer uses")
        mode = LN_STREAM_IN
    elif x.dtype != gamma.dtype:
        raise L.CogviewHipError(f"Sandwich-LN input {x.dtype} vs parameters {gamma.dtype}")
    y = torch.empty((rows, h), dtype=ydt, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    # algorithmic HBM bytes: x + y (+ residual), each in its own width
    nbytes = rows * h * (x2.element_size() + y.element_size() + (r2.element_size() if r2 is not None else 0))
    with timed_launch("layernorm", 0.0, nbytes, lambda: "ln_fwd " + _LN_MODE_NAME[mode] + (" + residual" if r2 is not None and mode == LN_ALL_T else "")):
        L.check(L.lib().cogv_sandwich_ln_fwd(dt_code(gamma), _p(x2), _p(gamma), _p(beta), _p(r2), _p(y), _p(mean), _p(rstd),
                                             _p(absmax_in), _p(absmax_out), rows, h, float(eps), mode, _stream()),
                "cogv_sandwich_ln_fwd")
    return y.view(x.shape), mean, rstd


def sandwich_ln_bwd(dy, x, gamma, mean, rstd, add_in=None, dropout=None, dgamma=None, dbeta=None, colsum=None,
                    accumulate=False, marked=False):
    """dx = [add_in +] mask(LN'(dy)).  dgamma/dbeta/colsum: preallocated [h] tensors (or None).
    marked: x is the output of a gemm(..., dropout=...) -- its dropped elements are -0.0 and no kept element is -0.0, so
    the mask is read from x (cogv_sandwich_ln_bwd_marked) instead of being regenerated from (seed, stream); `dropout`
    still supplies p.  Bit-identical to the regenerating form on such an x.
    Stream forms by dtype, mirroring sandwich_ln_fwd: fp32 `x` (LN1, LN2: the saved stream) -> dx fp32, add_in fp32;
    fp32 `dy` (LN3, LN4: the stream's gradient) with a 16-bit x -> dx 16-bit."""
    _need_gpu(dy, x)
    h = x.shape[-1]
    dy2, x2 = dy.reshape(-1, h), x.reshape(-1, h)
    assert dy2.is_contiguous() and x2.is_contiguous()
    rows = x2.shape[0]
    mode = LN_ALL_T
    if x.dtype == torch.float32:
        mode = LN_STREAM_IN
        if dy.dtype != gamma.dtype or (add_in is not None and add_in.dtype != torch.float32):
            raise L.CogviewHipError("Sandwich-LN backward (stream input): dy must be 16-bit and add_in fp32")
    elif dy.dtype == torch.float32:
        mode = LN_STREAM_OUT
        if add_in is not None and add_in.dtype != x.dtype:
            raise L.CogviewHipError("Sandwich-LN backward (stream output): add_in must have x's type")
    elif dy.dtype != x.dtype or (add_in is not None and add_in.dtype != x.dtype):
        raise L.CogviewHipError("Sandwich-LN backward: mixed 16-bit types")
    dx = torch.empty_like(x2)
    a2 = None
    if add_in is not None:
        a2 = add_in.reshape(-1, h)
        assert a2.is_contiguous()
    lib = L.lib()
    nbytes = lib.cogv_ln_bwd_workspace_bytes(rows, h)
    ws = workspace("ln_bwd", nbytes, x.device)
    p, seed, sid = (0.0, 0, 0) if dropout is None else dropout
    nb = rows * h * (dy2.element_size() + x2.element_size() + dx.element_size() + (a2.element_size() if a2 is not None else 0))
    marked = bool(marked) and p > 0.0
    if marked and mode == LN_STREAM_IN:
        raise L.CogviewHipError("Sandwich-LN backward: marked zeros need a 16-bit x")
    label = lambda: "ln_bwd " + _LN_MODE_NAME[mode] + ((" + dropout from marked zeros" if marked else " + dropout replay") if p > 0.0 else "") + \
        (" + add" if a2 is not None else "")
    # the marked entry point is the replaying one without (seed, stream)
    name, replay = ("cogv_sandwich_ln_bwd_marked", ()) if marked else ("cogv_sandwich_ln_bwd", (int(seed), int(sid)))
    with timed_launch("layernorm", 0.0, nb, label):
        L.check(getattr(lib, name)(dt_code(gamma), _p(dy2), _p(x2), _p(gamma), _p(mean), _p(rstd), _p(a2), _p(dx), _p(dgamma), _p(dbeta),
                                   _p(colsum), int(accumulate), rows, h, float(p), *replay, _p(ws), ws.numel(), mode, _stream()), name)
    return dx.view(x.shape)


def ln_bwd_pair_supported(h):
    """cogv_sandwich_ln_bwd_pair takes rows of at least four waves of 8-column lanes (h >= 1537 .. 4096)."""
    return 1536 < h <= 4096


def sandwich_ln_bwd_pair(dc, y, gamma2, mean2, rstd2, dout, ao, gamma3, mean3, rstd3, dropout_p=0.0, dgamma2=None, dbeta2=None,
                         dgamma3=None, dbeta3=None, colsum=None, accumulate=False):
    """LN2' and LN3' of a layer in one pass (cogv_sandwich_ln_bwd_pair): dy = dout + LN2'(dc; y) (fp32), d_ao = mask(LN3'(dy; ao))
    (16-bit; dropout_p > 0: ao carries the producing GEMM's marked zeros).  Returns (dy, d_ao); both bit-identical to
    sandwich_ln_bwd(dc, y, ..., add_in=dout) followed by sandwich_ln_bwd(dy, ao, ..., marked=True)."""
    _need_gpu(dc, y, ao)
    h = y.shape[-1]
    dc2, y2, do2, ao2 = dc.reshape(-1, h), y.reshape(-1, h), dout.reshape(-1, h), ao.reshape(-1, h)
    assert dc2.is_contiguous() and y2.is_contiguous() and do2.is_contiguous() and ao2.is_contiguous()
    if y.dtype != torch.float32 or dout.dtype != torch.float32 or dc.dtype != gamma2.dtype or ao.dtype != gamma2.dtype:
        raise L.CogviewHipError("Sandwich-LN backward pair: y / dout must be the fp32 stream, dc / ao the 16-bit storage type")
    rows = y2.shape[0]
    dy = torch.empty_like(y2)
    d_ao = torch.empty_like(ao2)
    lib = L.lib()
    ws = workspace("ln_bwd_pair", lib.cogv_ln_bwd_pair_workspace_bytes(rows, h), y.device)
    nb = rows * h * (2 + 4 + 4 + 4 + 2 + 2)
    with timed_launch("layernorm", 0.0, nb, lambda: "ln_bwd pair: stream in + add, then stream out" + (" + dropout from marked zeros" if dropout_p > 0.0 else "")):
        L.check(lib.cogv_sandwich_ln_bwd_pair(dt_code(gamma2), _p(dc2), _p(y2), _p(gamma2), _p(mean2), _p(rstd2), _p(do2), _p(dy),
                                              _p(dgamma2), _p(dbeta2), _p(ao2), _p(gamma3), _p(mean3), _p(rstd3), _p(d_ao),
                                              _p(dgamma3), _p(dbeta3), _p(colsum), int(accumulate), rows, h, float(dropout_p),
                                              _p(ws), ws.numel(), _stream()), "cogv_sandwich_ln_bwd_pair")
    return dy.view(y.shape), d_ao.view(ao.shape)


# ------------------------------------------------------------------------------------------ attention
def attention_executed_flops(b, H, s_q, s_k, sep=0, dense=True):
    """FLOPs the forward attention kernel EXECUTES: 64 x 64 score blocks that hold at least one visible key (left-to-right rule
    with the fully visible prefix `sep`; a masked block is skipped, a diagonal block computed whole), 2 products of
    2 * 64 * 64 * 64 FLOPs each.  s = 1088: 153 of 289 blocks ("causal-discounted").  Forms that visit
    every block (arbitrary mask tensors, gathered / sparse keys) count all of them."""
    nq, nk = (s_q + 63) // 64, (s_k + 63) // 64
    if dense:
        off = s_k - s_q
        sep_i = int(sep) if isinstance(sep, int) else 0
        blocks = 0
        for i in range(nq):
            last_key = max(min(s_q, 64 * i + 64) - 1 + off, sep_i - 1)        # last visible key of the block's last query
            blocks += max(0, min(nk, last_key // 64 + 1))
    else:
        blocks = nq * nk
    return float(b) * H * blocks * 4.0 * 64 * 64 * 64


def _attn_strides(t):
    # t: [b, s, heads, 64] view with d contiguous and heads packed (stride 64)
    assert t.dim() == 4 and t.shape[-1] == 64 and t.stride(3) == 1 and (t.stride(2) == 64 or t.shape[2] == 1)
    return t.stride(0), t.stride(1)


def _attn_desc(q, k, v, o, sep, dropout):
    d = L.AttnDesc()
    d.dtype = dt_code(q)
    d.B, d.s_q, d.H = q.shape[0], q.shape[1], q.shape[2]
    d.s_k = k.shape[1]
    d.head_dim = 64
    d.sep = int(sep)
    d.scale = 0.125
    p, seed, sid = (0.0, 0, 0) if dropout is None else dropout
    d.dropout_p, d.seed, d.stream_id = float(p), int(seed), int(sid)
    d.q, d.k, d.v, d.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    d.q_bs, d.q_rs = _attn_strides(q)
    d.k_bs, d.k_rs = _attn_strides(k)
    d.v_bs, d.v_rs = _attn_strides(v)
    d.o_bs, d.o_rs = _attn_strides(o)
    return d


STORE_KEEP_BITS = os.environ.get("COGV_ATTN_KEEP_BITS", "1") != "0"       # A/B switch of the stored dropout keep bits


def _attn_mask(d, mask, q, k):
    """mask: [B or 1, s_q, s_k] contiguous, q's dtype -- an arbitrary mask tensor (cogv_attn_desc.mask)."""
    b, s_q, s_k = q.shape[0], q.shape[1], k.shape[1]
    assert mask.dtype == q.dtype and mask.is_contiguous() and mask.dim() == 3 and mask.shape[1:] == (s_q, s_k)
    assert mask.shape[0] in (1, b)
    d.mask, d.mask_bs = mask.data_ptr(), (s_q * s_k if mask.shape[0] == b and b > 1 else 0)


def attention_fwd(q, k, v, sep=0, dropout=None, kv_index=None, sparse=None, keep_bits=False, mask=None):
    """q [b,s_q,H,64], k/v [b,s_k,H,64] (strided views are fine).  Returns (o [b,s_q,H,64] contiguous, lse).
    keep_bits=True (dense form with dropout; the caller will run attention_bwd): returns (o, lse, bits) -- the forward
    kernel stores its dropout keep decisions (1 bit per score, uint8 buffer of cogv_attention_keep_bits_bytes) and
    attention_bwd(keep_bits=bits) reads them instead of regenerating the draws; bits is None where that does not apply.
    kv_index [b, n] int32 (forward only): key slot j is row kv_index[b, j] of k / v -- the gathered form of
    sparse_attention_inference; the left-to-right rule then applies to slots (the last s_q slots are the queries)."""
    _need_gpu(q, k, v)
    b, s_q, H, _ = q.shape
    o = torch.empty((b, s_q, H, 64), dtype=q.dtype, device=q.device)
    lse = torch.empty((b, H, s_q), dtype=torch.float32, device=q.device)
    d = _attn_desc(q, k, v, o, sep, dropout)
    if kv_index is not None and sparse is None:
        assert kv_index.dtype == torch.int32 and kv_index.dim() == 2 and kv_index.shape[0] == b and kv_index.is_contiguous()
        assert kv_index.shape[1] >= s_q
        d.s_k = kv_index.shape[1]
        d.kv_index, d.kv_index_bs = kv_index.data_ptr(), kv_index.stride(0)
    elif sparse is not None:
        _sparse_desc(d, kv_index, sparse, b, s_q)
    d.lse = lse.data_ptr()
    bits = None
    if mask is not None:
        assert kv_index is None and sparse is None
        _attn_mask(d, mask, q, k)
    if keep_bits and STORE_KEEP_BITS and dropout is not None and dropout[0] > 0.0 and kv_index is None and sparse is None and mask is None:
        bits = torch.empty(L.lib().cogv_attention_keep_bits_bytes(b, H, s_q, k.shape[1]), dtype=torch.uint8, device=q.device)
        d.keep_bits = bits.data_ptr()
    with timed_launch("attention", lambda: attention_executed_flops(b, H, s_q, d.s_k, sep, dense=(kv_index is None and sparse is None and mask is None)),
                      0.0, lambda: f"attn_fwd {b}x{H}x{s_q}x{d.s_k}" + (" dropout" if dropout is not None else "")):
        L.check(L.lib().cogv_attention_fwd(C.byref(d), _stream()), "cogv_attention_fwd")
    return (o, lse, bits) if keep_bits else (o, lse)


_DECODE_WS = {}


def _decode_first(first, b, dev):
    """The `first` argument of the decode attentions: int32 [b] on the device, one first attended slot per cache row."""
    if first is None:
        return None
    _need_gpu(first)
    assert first.dtype == torch.int32 and first.numel() == b and first.is_contiguous() and first.device == dev
    return first.data_ptr()


def _decode_desc(d, qkv, pos_index, b, heads, cap, combine, first, rows=None, out_shape=None):
    """What the decode attentions share: (descriptor with every field but the cache's, out or None, workspace).  The
    workspace (partial results of the key splits) is kept per (device, rows, heads, capacity): fixed addresses, so the call is
    replayable inside a captured graph.  rows, out_shape: of a chunk step (b * m rows, out [b, m, heads * 64]; the caller sets
    m and the row strides); None: one row per cache row."""
    hp = heads * 64
    key = (qkv.device.index, rows or b, heads, cap)
    ws = _DECODE_WS.get(key)
    if ws is None:
        ws = _DECODE_WS[key] = torch.zeros(L.lib().cogv_attention_decode_workspace_bytes(rows or b, heads, cap), dtype=torch.uint8, device=qkv.device)
    out = torch.empty(out_shape or (b, 1, hp), dtype=qkv.dtype, device=qkv.device) if combine else None
    d.dtype, d.B, d.H, d.capacity, d.head_dim, d.scale = dt_code(qkv), b, heads, cap, 64, 0.125
    d.qkv, d.out = qkv.data_ptr(), out.data_ptr() if combine else None
    if out_shape is None:
        d.qkv_bs, d.out_bs = qkv.stride(0), hp
    d.pos = pos_index.data_ptr()
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    d.skip_combine = 0 if combine else 1
    d.first = _decode_first(first, b, qkv.device)
    return d, out, ws


def attention_decode(qkv, cache, pos_index, heads, combine=True, first=None):
    """combine=False: only the key-split kernel runs; returns the partials workspace for gemv_attn (the attention-output
    projection recombines the splits in its prologue: one launch less).
    One decode step's attention (cogv_attention_decode): qkv [b, 1, 3 * heads * 64] (q | k | v of the new token),
    cache [b, capacity, 2 * heads * 64] (keys | values), pos_index: device int64 scalar = slot of the new token (slots
    [0, pos] are attended; the new key / value are written into slot pos by the kernel).  Returns out [b, 1, heads * 64].
    first: device int32 [b] -- row r attends slots [first[r], pos] (rows with right-aligned contexts of different lengths;
    the slots below first[r] are padding and may hold anything).  None: the launch without it."""
    _need_gpu(qkv, cache, pos_index)
    b, cap = cache.shape[0], cache.shape[1]
    hp = heads * 64
    assert qkv.shape[0] == b and qkv.shape[-1] == 3 * hp and qkv.numel() == b * 3 * hp and cache.shape[2] == 2 * hp
    assert qkv.stride(-1) == 1 and cache.stride(2) == 1 and pos_index.dtype == torch.int64
    d, out, ws = _decode_desc(L.AttnDecodeDesc(), qkv, pos_index, b, heads, cap, combine, first)
    d.cache, d.cache_bs, d.cache_rs = cache.data_ptr(), cache.stride(0), cache.stride(1)
    L.check(L.lib().cogv_attention_decode(C.byref(d), _stream()), "cogv_attention_decode")
    return out if combine else ws


def attention_decode_chunk(qkv, cache, pos_index, heads, combine=True, first=None):
    """attention_decode for m tokens per cache row (cogv_attention_decode_chunk): qkv [b, m, 3 * heads * 64] with 1 <= m <= 8
    (rows r = b * m + j, as the QKV projection of [b * m, h] hidden rows leaves them), cache and pos_index as there.  Row
    (b, j) is the token of slot pos + j and attends slots [first[b], pos + j]; the m keys / values are written into slots
    [pos, pos + m) (none at or past the capacity).  Returns out [b, m, heads * 64], or with combine=False the partials of b * m
    rows for gemv_attn(partials, b * m, ...).  Bit-identical to m attention_decode calls at pos, pos + 1, ..."""
    _need_gpu(qkv, cache, pos_index)
    b, cap = cache.shape[0], cache.shape[1]
    hp = heads * 64
    assert qkv.dim() == 3 and qkv.shape[0] == b and qkv.shape[2] == 3 * hp and cache.shape[2] == 2 * hp
    m = qkv.shape[1]
    assert qkv.stride(2) == 1 and (b == 1 or qkv.stride(0) == m * qkv.stride(1)), "rows b * m + j one stride apart"
    assert cache.stride(2) == 1 and pos_index.dtype == torch.int64
    d, out, ws = _decode_desc(L.AttnDecodeChunkDesc(), qkv, pos_index, b, heads, cap, combine, first, rows=b * m, out_shape=(b, m, hp))
    d.m, d.qkv_rs, d.out_rs = m, qkv.stride(1), hp
    d.cache, d.cache_bs, d.cache_rs = cache.data_ptr(), cache.stride(0), cache.stride(1)
    L.check(L.lib().cogv_attention_decode_chunk(C.byref(d), _stream()), "cogv_attention_decode_chunk")
    return out if combine else ws


def kv_quantize_e4m3(kv, q, scale, slot0=0):
    """cogv_kv_quantize_e4m3: the 16-bit K | V rows a prefill leaves, kv [b, n, 2 * heads * 64] (batch and row strides free),
    into slots [slot0, slot0 + n) of an 8-bit cache: q [b, 2, heads, capacity, 64] uint8 (OCP E4M3 bytes; plane 0 keys, plane 1
    values) and scale [b, 2, heads, capacity] fp32, one scale per (slot, head, K | V) = abs-max of its 64 elements / 448 (1.0
    when they are all zero), q = rne_e4m3(x.float() / scale).  q / scale may be the leading rows of a larger cache."""
    _need_gpu(kv, q, scale)
    assert kv.dim() == 3 and kv.stride(2) == 1 and q.dim() == 5 and scale.dim() == 4
    b, n, w = kv.shape
    heads, cap = q.shape[2], q.shape[3]
    assert w == 2 * heads * 64 and q.shape == (b, 2, heads, cap, 64) and scale.shape == (b, 2, heads, cap)
    assert q.dtype == torch.uint8 and scale.dtype == torch.float32 and q[0].is_contiguous() and scale[0].is_contiguous()
    assert 0 <= slot0 and slot0 + n <= cap
    L.check(L.lib().cogv_kv_quantize_e4m3(dt_code(kv), _p(kv), kv.stride(0), kv.stride(1), b, n, heads, _p(q), q.stride(0), _p(scale),
                                          scale.stride(0), cap, int(slot0), _stream()), "cogv_kv_quantize_e4m3")


def attention_decode_kv8(qkv, cache8, pos_index, heads, combine=True, first=None):
    """attention_decode on an 8-bit cache (cogv_attention_decode_kv8): cache8 = (q [b, 2, heads, capacity, 64] uint8,
    scale [b, 2, heads, capacity] fp32) as kv_quantize_e4m3 fills it, or an object with these as .q / .scale (StaticKV8Slot).  The new token's key / value are quantized, written into
    slot pos as bytes + scale, and attended in their dequantized form.  Result, partials (combine=False) and the workspace
    cache (keyed as attention_decode's: the same buffers) as there; `first` as there (bytes and scales of the padding slots
    may hold anything)."""
    q, scale = (cache8.q, cache8.scale) if hasattr(cache8, "scale") else cache8
    _need_gpu(qkv, q, scale, pos_index)
    b, cap = q.shape[0], q.shape[3]
    hp = heads * 64
    assert qkv.shape[0] == b and qkv.shape[-1] == 3 * hp and qkv.numel() == b * 3 * hp and qkv.stride(-1) == 1
    assert q.dtype == torch.uint8 and q.shape == (b, 2, heads, cap, 64) and q[0].is_contiguous()
    assert scale.dtype == torch.float32 and scale.shape == (b, 2, heads, cap) and scale[0].is_contiguous()
    assert pos_index.dtype == torch.int64
    d, out, ws = _decode_desc(L.AttnDecodeKv8Desc(), qkv, pos_index, b, heads, cap, combine, first)
    d.kv_q, d.kv_q_bs = q.data_ptr(), q.stride(0)
    d.kv_scale, d.kv_scale_bs = scale.data_ptr(), scale.stride(0)
    L.check(L.lib().cogv_attention_decode_kv8(C.byref(d), _stream()), "cogv_attention_decode_kv8")
    return out if combine else ws


def attention_decode_chunk_kv8(qkv, cache8, pos_index, heads, combine=True, first=None):
    """attention_decode_chunk on an 8-bit cache (cogv_attention_decode_chunk_kv8): qkv [b, m, 3 * heads * 64] with 1 <= m <= 8,
    output and workspace as attention_decode_chunk's; cache8 as attention_decode_kv8's.  The chunk's m keys / values are
    quantized, written into slots [pos, pos + m) as bytes + scales (none at or past the capacity), and attended in their
    dequantized form; row (b, j) attends slots [first[b], pos + j].  Returns out [b, m, heads * 64], or with combine=False the
    partials of b * m rows.  Bit-identical (outputs, partials, cache) to m attention_decode_kv8 calls at pos, pos + 1, ..."""
    q, scale = (cache8.q, cache8.scale) if hasattr(cache8, "scale") else cache8
    _need_gpu(qkv, q, scale, pos_index)
    b, cap = q.shape[0], q.shape[3]
    hp = heads * 64
    assert qkv.dim() == 3 and qkv.shape[0] == b and qkv.shape[2] == 3 * hp
    m = qkv.shape[1]
    assert qkv.stride(2) == 1 and (b == 1 or qkv.stride(0) == m * qkv.stride(1)), "rows b * m + j one stride apart"
    assert q.dtype == torch.uint8 and q.shape == (b, 2, heads, cap, 64) and q[0].is_contiguous()
    assert scale.dtype == torch.float32 and scale.shape == (b, 2, heads, cap) and scale[0].is_contiguous()
    assert pos_index.dtype == torch.int64
    d, out, ws = _decode_desc(L.AttnDecodeChunkKv8Desc(), qkv, pos_index, b, heads, cap, combine, first, rows=b * m, out_shape=(b, m, hp))
    d.m, d.qkv_rs, d.out_rs = m, qkv.stride(1), hp
    d.kv_q, d.kv_q_bs = q.data_ptr(), q.stride(0)
    d.kv_scale, d.kv_scale_bs = scale.data_ptr(), scale.stride(0)
    L.check(L.lib().cogv_attention_decode_chunk_kv8(C.byref(d), _stream()), "cogv_attention_decode_chunk_kv8")
    return out if combine else ws


def gemv_attn(partials, batch, heads, capacity, w, bias=None, absmax=None):
    """Attention-output projection of a decode step with the split-combine as its prologue (cogv_gemv_attn):
    out [batch, N] = (combined attention output [batch, heads * 64]) . w^T + bias.  `partials`: what
    attention_decode(..., combine=False) returned for the same (batch, heads, capacity)."""
    _need_gpu(partials, w)
    N, K = w.shape
    assert K == heads * 64 and w.stride(1) == 1 and batch <= 8
    out = torch.empty((batch, N), dtype=w.dtype, device=w.device)
    d = _skinny_desc(out, K, bias, False, absmax)
    d.B, d.ldb = w.data_ptr(), w.stride(0)
    L.check(L.lib().cogv_gemv_attn(C.byref(d), _p(partials), int(heads), int(capacity), _stream()), "cogv_gemv_attn")
    return out


# ------------------------------------------------------------------------------------------ 8-bit weights (decode step)
def quantize_rows_e4m3(w):
    """cogv_quantize_rows_e4m3: w [N, K] fp16 / bf16 (rows may be strided) -> (q [N, K] uint8: OCP E4M3 bytes, scale [N] fp32)
    with scale = row abs-max / 448 (1.0 for a zero row) and q = rne_e4m3(w.float() / scale) -- the weight operand of gemm_w8,
    gemv_ln_w8 and gemv_attn_w8.  View q as torch.float8_e4m3fn to read the values."""
    _need_gpu(w)
    assert w.dim() == 2 and w.stride(1) == 1
    N, K = w.shape
    q = torch.empty((N, K), dtype=torch.uint8, device=w.device)
    scale = torch.empty(N, dtype=torch.float32, device=w.device)
    L.check(L.lib().cogv_quantize_rows_e4m3(dt_code(w), _p(w), w.stride(0), N, K, _p(q), K, _p(scale), _stream()),
            "cogv_quantize_rows_e4m3")
    return q, scale


def _q_call(fmt, x_dtype, M, K, qs, bias, gelu, absmax):
    """(descriptor, operand, out) of a skinny-M product on the quantized weight qs = (q, scale) of format `fmt`."""
    N, K, w = _q_operand(fmt, qs, K)
    assert bias is None or bias.dtype == x_dtype
    out = torch.empty((M, N), dtype=x_dtype, device=qs[0].device)
    return _skinny_desc(out, K, bias, gelu, absmax), w, out


def _w8_call(x_dtype, M, K, qs, bias, gelu, absmax):
    """_q_call on the E4M3 weight (tests/test_gemv_cells_gpu.py fills the descriptor and the operand itself around it)"""
    return _q_call("e4m3", x_dtype, M, K, qs, bias, gelu, absmax)


# the three skinny-M kinds on a quantized weight of format `fmt`; the public functions below bind it
def _gemm_q(fmt, a, qs, bias, gelu, absmax):
    _need_gpu(a)
    assert a.dim() == 2 and a.stride(1) == 1
    M, K = a.shape
    d, w, out = _q_call(fmt, a.dtype, M, K, qs, bias, gelu, absmax)
    d.A, d.lda = a.data_ptr(), a.stride(0)
    name = "cogv_gemm" + _Q_SUFFIX[fmt]
    L.check(getattr(L.lib(), name)(C.byref(d), C.byref(w), _stream()), name)
    return out


def _gemv_ln_q(fmt, z, qs, bias, gamma, beta, eps, z_absmax, post, residual, want_t, gelu, absmax):
    _need_gpu(z, gamma)
    assert z.dim() == 2 and z.is_contiguous()
    M, K = z.shape
    d, w, out = _q_call(fmt, gamma.dtype, M, K, qs, bias, gelu, absmax)
    ln, t = _ln_prologue(z, gamma, beta, eps, z_absmax, post, residual, want_t)
    name = "cogv_gemv_ln" + _Q_SUFFIX[fmt]
    L.check(getattr(L.lib(), name)(C.byref(d), C.byref(ln), C.byref(w), _stream()), name)
    return out, t


def _gemv_attn_q(fmt, partials, batch, heads, capacity, qs, dtype, bias, absmax):
    _need_gpu(partials)
    assert batch <= 8
    d, w, out = _q_call(fmt, dtype, batch, heads * 64, qs, bias, False, absmax)
    name = "cogv_gemv_attn" + _Q_SUFFIX[fmt]
    L.check(getattr(L.lib(), name)(C.byref(d), C.byref(w), _p(partials), int(heads), int(capacity), _stream()), name)
    return out


def gemm_w8(a, qs, bias=None, gelu=False, absmax=None):
    """gemm's skinny case (a [M, K], M <= 8) on an 8-bit weight qs = (q [N, K] uint8, scale [N]) from quantize_rows_e4m3
    (cogv_gemm_w8): out [M, N] = epilogue(scale * (a . e4m3(q)^T) + bias) in a's dtype.  Shapes outside the kernels' classes raise:
    there is no other kernel behind this one."""
    return _gemm_q("e4m3", a, qs, bias, gelu, absmax)


def gemv_ln_w8(z, qs, bias, gamma, beta, eps, z_absmax=None, post=None, residual=None, want_t=False, gelu=False, absmax=None):
    """gemv_ln on an 8-bit weight qs = (q, scale) (cogv_gemv_ln_w8); everything else as there.  The output takes gamma's dtype."""
    return _gemv_ln_q("e4m3", z, qs, bias, gamma, beta, eps, z_absmax, post, residual, want_t, gelu, absmax)


def gemv_attn_w8(partials, batch, heads, capacity, qs, dtype, bias=None, absmax=None):
    """gemv_attn on an 8-bit weight qs = (q, scale) (cogv_gemv_attn_w8); `dtype`: the 16-bit type of the output (and bias)."""
    return _gemv_attn_q("e4m3", partials, batch, heads, capacity, qs, dtype, bias, absmax)


# ------------------------------------------------------------------------------------------ 4-bit weights (decode step)
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def quantize_rows_mxfp4(w):
    """cogv_quantize_rows_mxfp4: w [N, K] fp16 / bf16 (K % 32 == 0, rows may be strided) -> (q [N, K / 2] uint8: two E2M1 codes per
    byte, element 2i in the low nibble of byte i; scale [N, K / 32] uint8: one E8M0 exponent per block of 32, value 2^(scale - 127))
    by the OCP MXFP4 rule of include/cogview_hip.h -- the weight operand of gemm_w4, gemv_ln_w4 and gemv_attn_w4.
    dequantize_rows_mxfp4 reads the values back."""
    _need_gpu(w)
    assert w.dim() == 2 and w.stride(1) == 1 and w.shape[1] % 32 == 0
    N, K = w.shape
    q = torch.empty((N, K // 2), dtype=torch.uint8, device=w.device)
    scale = torch.empty((N, K // 32), dtype=torch.uint8, device=w.device)
    L.check(L.lib().cogv_quantize_rows_mxfp4(dt_code(w), _p(w), w.stride(0), N, K, _p(q), q.stride(0), _p(scale), scale.stride(0), _stream()),
            "cogv_quantize_rows_mxfp4")
    return q, scale


def dequantize_rows_mxfp4(q, scale, dtype=torch.float32):
    """The values an MXFP4 pair holds, in plain torch on any device: q [N, K / 2] uint8, scale [N, K / 32] uint8 -> [N, K] `dtype`
    = sign * E2M1[code] * 2^(scale - 127).  Exact in fp32 (the default), fp64 and bf16; in fp16 wherever the value is a multiple
    of 2^-24 below 65520."""
    assert q.dtype == torch.uint8 and scale.dtype == torch.uint8 and q.dim() == 2 and q.shape[1] == scale.shape[1] * 16
    nib = torch.stack((q & 15, q >> 4), dim=-1).reshape(q.shape[0], -1).long()
    mag = torch.tensor(_E2M1, dtype=torch.float64, device=q.device)[nib & 7]
    val = torch.where((nib & 8) != 0, -mag, mag)
    return torch.ldexp(val, (scale.long() - 127).repeat_interleave(32, dim=1)).to(dtype)


def gemm_w4(a, qs, bias=None, gelu=False, absmax=None):
    """gemm's skinny case (a [M, K], M <= 8) on a 4-bit weight qs = (q [N, K / 2] uint8, scale [N, K / 32] uint8) from
    quantize_rows_mxfp4 (cogv_gemm_w4): out [M, N] = epilogue(a . dequantize_rows_mxfp4(q, scale)^T + bias) in a's dtype.  Shapes
    outside the kernels' classes raise: there is no other kernel behind this one."""
    return _gemm_q("mxfp4", a, qs, bias, gelu, absmax)


def gemv_ln_w4(z, qs, bias, gamma, beta, eps, z_absmax=None, post=None, residual=None, want_t=False, gelu=False, absmax=None):
    """gemv_ln on a 4-bit weight qs = (q, scale) (cogv_gemv_ln_w4); everything else as there.  The output takes gamma's dtype."""
    return _gemv_ln_q("mxfp4", z, qs, bias, gamma, beta, eps, z_absmax, post, residual, want_t, gelu, absmax)


def gemv_attn_w4(partials, batch, heads, capacity, qs, dtype, bias=None, absmax=None):
    """gemv_attn on a 4-bit weight qs = (q, scale) (cogv_gemv_attn_w4); `dtype`: the 16-bit type of the output (and bias)."""
    return _gemv_attn_q("mxfp4", partials, batch, heads, capacity, qs, dtype, bias, absmax)


def _sparse_desc(d, kv_index, sparse, b, s_q):
    """Sparse training form in slot space: kv_index [b, s_q // w, n_slots] int32 (bit 31 = masked slot),
    sparse = (w, n_pivots, pivot_bias)."""
    w, n_piv, bias = sparse
    assert kv_index.dtype == torch.int32 and kv_index.dim() == 3 and kv_index.is_contiguous()
    assert kv_index.shape[0] == b and kv_index.shape[1] == s_q // w and s_q % w == 0 and w % 128 == 0
    d.s_k = kv_index.shape[2]
    d.kv_index, d.kv_index_bs, d.kv_index_gs = kv_index.data_ptr(), kv_index.stride(0), kv_index.stride(1)
    d.sparse_window, d.sparse_pivots, d.sparse_pivot_bias = int(w), int(n_piv), float(bias)


def sparse_attention_bwd(dout, q, k, v, o, lse, kv_index, sparse, pivot_inv, times, dropout=None):
    """Backward of the sparse training form (attention_fwd with sparse=...).  The dK/dV kernel works per (batch, query
    block) on the block's slots and leaves slot-space gradients; cogv_sparse_slot_reduce folds them onto the keys.
    pivot_inv [b, s] int32: pivot slot of each key or -1."""
    _need_gpu(dout, q, k, v, o)
    b, s, H, _ = q.shape
    w, n_piv, _bias = sparse
    G, n_slots = s // w, kv_index.shape[2]
    assert n_slots == n_piv + times * w and pivot_inv.dtype == torch.int32 and pivot_inv.shape == (b, s) and pivot_inv.is_contiguous()
    dq = torch.empty((b, s, H, 64), dtype=q.dtype, device=q.device)
    dks = torch.empty((b * G, n_slots, H, 64), dtype=q.dtype, device=q.device)
    dvs = torch.empty_like(dks)
    dvec = torch.empty((2, b, H, s), dtype=torch.float32, device=q.device)
    d = _attn_desc(q, k, v, o, 0, dropout)
    _sparse_desc(d, kv_index, sparse, b, s)
    d.lse, d.dvec = lse.data_ptr(), dvec.data_ptr()
    d.dout, d.dq, d.dk, d.dv = dout.data_ptr(), dq.data_ptr(), dks.data_ptr(), dvs.data_ptr()
    d.do_bs, d.do_rs = _attn_strides(dout)
    d.dq_bs, d.dq_rs = _attn_strides(dq)
    d.dk_bs, d.dk_rs = _attn_strides(dks)
    d.dv_bs, d.dv_rs = _attn_strides(dvs)
    L.check(L.lib().cogv_attention_bwd(C.byref(d), _stream()), "cogv_attention_bwd")
    dk = torch.empty((b, s, H, 64), dtype=q.dtype, device=q.device)
    dv = torch.empty_like(dk)
    L.check(L.lib().cogv_sparse_slot_reduce(dt_code(q), _p(dks), _p(dvs), _p(pivot_inv), _p(dk), _p(dv),
                                            dk.stride(0), dk.stride(1), dv.stride(0), dv.stride(1), b, s, H, int(w),
                                            int(times), int(n_piv), _stream()), "cogv_sparse_slot_reduce")
    return dq, dk, dv


def attention_bwd(dout, q, k, v, o, lse, sep=0, dropout=None, dq=None, dk=None, dv=None, colsum_out=None,
                  colsum_accumulate=True, keep_bits=None, mask=None):
    """colsum_out [3*H*64]: (+)= column sums of (dq | dk | dv) over all tokens -- the bias gradient of the fused
    QKV projection -- taken from the kernels' accumulators instead of re-reading the three outputs."""
    _need_gpu(dout, q, k, v, o)
    b, s_q, H, _ = q.shape
    if dq is None:
        dq = torch.empty((b, s_q, H, 64), dtype=q.dtype, device=q.device)
    if dk is None:
        dk = torch.empty((b, k.shape[1], H, 64), dtype=q.dtype, device=q.device)
    if dv is None:
        dv = torch.empty((b, k.shape[1], H, 64), dtype=q.dtype, device=q.device)
    dvec = torch.empty((2, b, H, s_q), dtype=torch.float32, device=q.device)
    d = _attn_desc(q, k, v, o, sep, dropout)
    d.lse, d.dvec = lse.data_ptr(), dvec.data_ptr()
    if mask is not None:
        _attn_mask(d, mask, q, k)
    if keep_bits is not None:
        assert mask is None and keep_bits.numel() == L.lib().cogv_attention_keep_bits_bytes(b, H, s_q, k.shape[1])
        d.keep_bits = keep_bits.data_ptr()
    d.dout, d.dq, d.dk, d.dv = dout.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    d.do_bs, d.do_rs = _attn_strides(dout)
    d.dq_bs, d.dq_rs = _attn_strides(dq)
    d.dk_bs, d.dk_rs = _attn_strides(dk)
    d.dv_bs, d.dv_rs = _attn_strides(dv)
    fuse = colsum_out is not None and k.shape[1] == s_q
    if fuse:
        rows = b * ((s_q + 127) // 128)
        ws = workspace("attn_colsum", rows * 3 * H * 64 * 4, q.device)
        d.colsum_partial = ws.data_ptr()
    # 5 block products against the forward's 2
    with timed_launch("attention", lambda: 2.5 * attention_executed_flops(b, H, s_q, k.shape[1], sep, dense=mask is None), 0.0,
                      lambda: f"attn_bwd {b}x{H}x{s_q}x{k.shape[1]} (D, dQ, dK.dV)" + (" dropout" if dropout is not None else "")):
        L.check(L.lib().cogv_attention_bwd(C.byref(d), _stream()), "cogv_attention_bwd")
    if fuse:
        L.check(L.lib().cogv_colsum_finalize(dt_code(q), d.colsum_partial, rows, 3 * H * 64, _p(colsum_out),
                                             int(colsum_accumulate), _stream()), "cogv_colsum_finalize")
    elif colsum_out is not None:
        for i, t in enumerate((dq, dk, dv)):
            colsum(t.reshape(-1, H * 64), out=colsum_out[i * H * 64:(i + 1) * H * 64], accumulate=colsum_accumulate)
    return dq, dk, dv


# ------------------------------------------------------------------------------------------ embedding
def embedding_fwd(ids, table, vocab_start, pos_ids=None, pos_table=None, dropout=None, absmax_out=None, x_in=None,
                  out_f32=False):
    """out_f32: the result is the transformer's fp32 residual stream (word + position summed in fp32)."""
    _need_gpu(table if table is not None else x_in)
    src = table if table is not None else x_in
    h = src.shape[-1]
    if ids is not None:
        ids_c = ids.contiguous()
        n_tok, shape = ids_c.numel(), tuple(ids.shape) + (h,)
    else:
        ids_c = None
        x_in = x_in.contiguous()
        n_tok, shape = x_in.numel() // h, tuple(x_in.shape)
    pos_c = None
    if pos_table is not None:
        pos_c = pos_ids.expand(shape[:-1]).contiguous()
    out = torch.empty(shape, dtype=torch.float32 if out_f32 else src.dtype, device=src.device)
    p, seed, sid = (0.0, 0, 0) if dropout is None else dropout
    vend = vocab_start + (table.shape[0] if table is not None else 0)
    L.check(L.lib().cogv_embedding_fwd(dt_code(src), _p(ids_c), _p(table), int(vocab_start), int(vend), _p(x_in),
                                       _p(pos_c), _p(pos_table), 0 if pos_table is None else pos_table.shape[0],
                                       _p(out), _p(absmax_out), n_tok, h, float(p), int(seed), int(sid), int(out_f32),
                                       _stream()), "cogv_embedding_fwd")
    return out


def embedding_bwd(dout, ids, dtable, vocab_start, pos_ids=None, dpos=None, dropout=None, dx=None):
    """dtable[id - vocab_start] += sum of the (masked) gradient rows of the tokens carrying id; dpos likewise.  fp32
    sums in ascending token order, one rounding, no floating-point atomics: deterministic.  dout (and dx) may be fp32
    (the residual stream's gradient) or the tables' 16-bit type."""
    _need_gpu(dout)
    h = dout.shape[-1]
    dout_c = dout.contiguous()
    n_tok = dout_c.numel() // h
    ids_c = None if ids is None else ids.contiguous()
    pos_c = None if pos_ids is None else pos_ids.expand(dout.shape[:-1]).contiguous()
    p, seed, sid = (0.0, 0, 0) if dropout is None else dropout
    vend = vocab_start + (dtable.shape[0] if dtable is not None else 0)
    tab = dtable if dtable is not None else dpos
    d32 = dout.dtype == torch.float32
    assert dx is None or dx.dtype == dout.dtype
    lib = L.lib()
    nbytes = lib.cogv_embedding_bwd_workspace_bytes(0 if dtable is None else dtable.shape[0], 0 if dpos is None else dpos.shape[0])
    ws = workspace("embedding_bwd", nbytes, dout.device) if nbytes else None
    L.check(lib.cogv_embedding_bwd(dt_code(tab if tab is not None else dout), _p(dout_c), _p(ids_c), _p(dtable),
                                   int(vocab_start), int(vend), _p(pos_c), _p(dpos), 0 if dpos is None else dpos.shape[0],
                                   _p(dx), n_tok, h, float(p), int(seed), int(sid), _p(ws), 0 if ws is None else ws.numel(),
                                   int(d32), _stream()), "cogv_embedding_bwd")


# ------------------------------------------------------------------------------------------ element-wise
def _flat(t):
    assert t.is_contiguous() and t.numel() % 8 == 0, "element-wise ops need contiguous tensors with numel % 8 == 0"
    return t


def gelu_fwd(x):
    _need_gpu(x)
    y = torch.empty_like(_flat(x))
    L.check(L.lib().cogv_gelu_fwd(dt_code(x), _p(x), _p(y), x.numel(), _stream()), "cogv_gelu_fwd")
    return y


def gelu_bwd(dy, x):
    _need_gpu(dy, x)
    dx = torch.empty_like(_flat(x))
    L.check(L.lib().cogv_gelu_bwd(dt_code(x), _p(_flat(dy)), _p(x), _p(dx), x.numel(), _stream()), "cogv_gelu_bwd")
    return dx


def dropout(x, p, seed, stream_id, absmax_out=None):
    _need_gpu(x)
    y = torch.empty_like(_flat(x))
    L.check(L.lib().cogv_dropout(dt_code(x), _p(x), _p(y), x.numel(), float(p), int(seed), int(stream_id),
                                 _p(absmax_out), _stream()), "cogv_dropout")
    return y


def add(a, b, absmax_out=None):
    """a + b.  An fp32 `a` is the residual stream joined by the 16-bit branch output `b` (fp32 result)."""
    _need_gpu(a, b)
    if b.dtype == torch.float32 and a.dtype != torch.float32:
        raise L.CogviewHipError("ops.add: the fp32 operand (the residual stream) must come first")
    assert a.numel() == b.numel()
    if a.dtype == torch.float32 and b.dtype != torch.float32:
        out = torch.empty_like(_flat(a))
        L.check(L.lib().cogv_add_stream(dt_code(b), _p(a), _p(_flat(b)), _p(out), a.numel(), _p(absmax_out), _stream()),
                "cogv_add_stream")
        return out
    out = torch.empty_like(_flat(a))
    L.check(L.lib().cogv_add(dt_code(a), _p(a), _p(_flat(b)), _p(out), a.numel(), _p(absmax_out), _stream()), "cogv_add")
    return out


def scale(x, s):
    _need_gpu(x)
    y = torch.empty_like(_flat(x))
    L.check(L.lib().cogv_scale(dt_code(x), _p(x), _p(y), x.numel(), float(s), _stream()), "cogv_scale")
    return y


def absmax(x, out=None):
    """atomicMax of |x| into `out` (a zeroed fp32 scalar; allocated when None)."""
    _need_gpu(x)
    assert x.is_contiguous()
    if out is None:
        out = new_absmax_slot(x.device)
    L.check(L.lib().cogv_absmax(dt_code(x), _p(x), x.numel(), _p(out), _stream()), "cogv_absmax")
    return out


def colsum(dy, out=None, accumulate=False):
    _need_gpu(dy)
    assert dy.dim() == 2 and dy.stride(1) == 1
    M, N = dy.shape
    if out is None:
        out = torch.empty(N, dtype=dy.dtype, device=dy.device)
        assert not accumulate
    lib = L.lib()
    ws = workspace("colsum", lib.cogv_colsum_workspace_bytes(M, N), dy.device)
    L.check(lib.cogv_colsum(dt_code(dy), _p(dy), M, N, dy.stride(0), _p(out), int(accumulate), _p(ws), ws.numel(),
                            _stream()), "cogv_colsum")
    return out


# ------------------------------------------------------------------------------------------ cross entropy
def ce_fwd(logits2d, target1d, vocab_start, want_loss=True):
    _need_gpu(logits2d, target1d)
    assert logits2d.dim() == 2 and logits2d.is_contiguous() and target1d.is_contiguous()
    rows, v = logits2d.shape
    f = lambda: torch.empty(rows, dtype=torch.float32, device=logits2d.device)
    rowmax, sumexp, pred = f(), f(), f()
    loss = f() if want_loss else None
    L.check(L.lib().cogv_ce_fwd(dt_code(logits2d), _p(logits2d), _p(target1d), int(vocab_start), rows, v, _p(rowmax),
                                _p(sumexp), _p(pred), _p(loss), _stream()), "cogv_ce_fwd")
    return rowmax, sumexp, pred, loss


def ce_bwd(logits2d, target1d, vocab_start, gmax, gsum, grad, out=None):
    _need_gpu(logits2d)
    rows, v = logits2d.shape
    if out is None:
        out = torch.empty_like(logits2d)
    L.check(L.lib().cogv_ce_bwd(dt_code(logits2d), _p(logits2d), _p(target1d), int(vocab_start), rows, v, _p(gmax),
                                _p(gsum), _p(grad), _p(out), _stream()), "cogv_ce_bwd")
    return out


# ------------------------------------------------------------------------------------------ optimizer
def grad_stats(flat_grads, chunk_start, chunk_len, chunk_norm, stats):
    _need_gpu(flat_grads)
    lib = L.lib()
    # the partial sums of the pass: scratch owned by this side of the C ABI, one buffer per (device, stream) so that two
    # streams running the pass concurrently do not share it
    # (keyed on the stream handle as an INT: _stream() is a ctypes.c_void_p, which '%x' refuses on any non-default stream)
    sid = int(torch.cuda.current_stream(flat_grads.device).cuda_stream or 0)
    ws = workspace("grad_stats_%x" % sid, lib.cogv_grad_stats_workspace_bytes(), flat_grads.device, floor=0)
    with timed_launch("grad_stats", 0.0, flat_grads.numel() * flat_grads.element_size(), "overflow flag + per-chunk sum of squares"):
        L.check(lib.cogv_grad_stats(dt_code(flat_grads), _p(flat_grads), _p(chunk_start), _p(chunk_len),
                                    _p(chunk_norm), chunk_start.numel(), _p(stats), _p(ws), ws.numel(), _stream()), "cogv_grad_stats")


def adamw_step(params, grads, master, exp_avg, exp_avg_sq, chunk_start, chunk_len, chunk_group, lrs, wds, beta1,
               beta2, eps, step, inv_loss_scale=1.0, max_grad_norm=0.0, stats=None, sumsq_override=None,
               bias_correction=True, adam_w_mode=True):
    _need_gpu(params, grads, master)
    d = L.AdamDesc()
    d.dtype = dt_code(params)
    d.params, d.grads = params.data_ptr(), grads.data_ptr()
    d.master, d.exp_avg, d.exp_avg_sq = master.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr()
    d.chunk_start, d.chunk_len, d.chunk_group = chunk_start.data_ptr(), chunk_len.data_ptr(), chunk_group.data_ptr()
    d.nchunks = chunk_start.numel()
    assert len(lrs) <= 8
    for i, (lr, wd) in enumerate(zip(lrs, wds)):
        d.lr[i], d.weight_decay[i] = float(lr), float(wd)
    d.beta1, d.beta2, d.eps = float(beta1), float(beta2), float(eps)
    d.beta1_d, d.beta2_d = float(beta1), float(beta2)
    d.step, d.bias_correction, d.adam_w_mode = int(step), int(bias_correction), int(adam_w_mode)
    d.inv_loss_scale, d.max_grad_norm = float(inv_loss_scale), float(max_grad_norm)
    d.stats = None if stats is None else stats.data_ptr()
    d.norm_sumsq_override = None if sumsq_override is None else sumsq_override.data_ptr()
    # algorithmic bytes per parameter: 16-bit gradient in, master + two moments read and written (3 x 8), 16-bit parameter out
    with timed_launch("adamw", 0.0, params.numel() * (2 * params.element_size() + 24), "fused unscale + clip + AdamW + 16-bit copy-out"):
        L.check(L.lib().cogv_adamw_step(C.byref(d), _stream()), "cogv_adamw_step")


def cast_flat(src_half, dst_f32):
    _need_gpu(src_half, dst_f32)
    L.check(L.lib().cogv_cast_flat(dt_code(src_half), _p(src_half), _p(dst_f32), src_half.numel(), _stream()),
            "cogv_cast_flat")


def cast_flat_back(src_f32, dst_half):
    _need_gpu(src_f32, dst_half)
    L.check(L.lib().cogv_cast_flat_back(dt_code(dst_half), _p(src_f32), _p(dst_half), src_f32.numel(), _stream()),
            "cogv_cast_flat_back")


# ------------------------------------------------------------------------------------------ token sampling
def sample_logits(logits, *, temperature=1.0, top_k=0, top_p=0.0, allow=None, seed=0, offset=0, rows=None, ids=None,
                  logp=None, scores=None, probs=False, decode=None):
    """One draw per row of `logits` ([rows, vocab] or [rows, 1, vocab]; fp16 / bf16 / fp32; last dim contiguous) after the
    reference's filter (generation/sampling.py:24-50, 168-186): x / temperature, ids outside `allow` = (lo, hi) masked,
    top-k (ties at the threshold kept), top-p (per row), softmax, inverse-CDF draw keyed (seed, offset, row).
    rows: number of draws when logits holds ONE row (row stride 0: `rows` draws from it).
    offset: int, or a device int64 [1] tensor, which the launch advances by one.
    ids / logp / scores: optional output tensors (int64 / fp32 / fp32 accumulator, [rows]).  probs=True also returns the
    filtered distribution [rows, vocab] fp32.
    decode: dict of the decode graph's buffers (generation/decoder.py SamplingDecoder): tok, pos, pos_index, table, counter,
    out_tokens (optional), out_base, given (optional: int64 [>= capacity] by sequence position, shared by all rows; where
    given[*pos_index + 1] >= 0 that id is fed instead of drawn, with logp 0 and no score.  Or int64 [rows, >= capacity] with
    a contiguous last dimension: one table per row, the row stride taken from the tensor -- row r is fed where
    given[r, *pos_index + 1] >= 0 and draws elsewhere, whatever the other rows do).
    Returns (ids, logp, probs or None).  Allocates nothing when every output is given (what a captured graph needs)."""
    v = logits.shape[-1]
    src = logits.reshape(-1, v) if logits.dim() != 2 else logits
    _need_gpu(src)
    assert src.stride(-1) == 1, "logits: the vocabulary dimension must be contiguous"
    dev = src.device
    n = src.shape[0] if rows is None else int(rows)
    if rows is not None and src.shape[0] != 1:
        raise ValueError("rows= broadcasts ONE row of logits")
    lo, hi = (0, v) if allow is None else (int(allow[0]), int(allow[1]))
    if not 0 <= lo < hi <= v:
        raise ValueError(f"allowed range {allow} outside [0, {v})")
    if not 0 <= int(top_k) <= hi - lo:
        raise ValueError(f"top_k = {top_k} must lie in [0, {hi - lo}]")
    if not temperature > 0 or not top_p >= 0:
        raise ValueError("temperature must be > 0 and top_p >= 0")
    if ids is None:
        ids = torch.empty(n, dtype=torch.int64, device=dev)
    if logp is None:
        logp = torch.empty(n, dtype=torch.float32, device=dev)
    pr = torch.empty((n, v), dtype=torch.float32, device=dev) if probs else None
    for name, t, dt in (("ids", ids, torch.int64), ("logp", logp, torch.float32), ("scores", scores, torch.float32)):
        if t is not None and (t.dtype != dt or t.numel() != n or not t.is_contiguous()):
            raise ValueError(f"{name}: want a contiguous {dt} tensor of {n} elements")
    d = L.SampleDesc()
    d.dtype, d.rows, d.vocab = dt_code(src), n, v
    d.row_stride = 0 if (rows is not None or n == 1) else src.stride(0)
    d.logits = src.data_ptr()
    d.temperature, d.top_k, d.top_p, d.allow_lo, d.allow_hi = float(temperature), int(top_k), float(top_p), lo, hi
    d.seed = int(seed) & ((1 << 64) - 1)
    if isinstance(offset, torch.Tensor):
        assert offset.dtype == torch.int64 and offset.numel() == 1 and offset.device == dev
        d.offset = offset.data_ptr()
    elif offset:
        off_t = torch.tensor([int(offset)], dtype=torch.int64, device=dev)     # read by the launch, not advanced
        d.offset = off_t.data_ptr()
    d.ids, d.logp, d.scores, d.probs = ids.data_ptr(), logp.data_ptr(), _ptr(scores), _ptr(pr)
    if decode is not None:
        tab = decode["table"]
        assert tab.dtype == torch.int32 and tab.is_contiguous() and tab.shape[0] == n
        for k in ("tok", "pos"):
            assert decode[k].dtype == torch.int64 and decode[k].numel() == n and decode[k].is_contiguous()
        d.tok, d.pos, d.pos_index = decode["tok"].data_ptr(), decode["pos"].data_ptr(), decode["pos_index"].data_ptr()
        d.table, d.capacity = tab.data_ptr(), tab.shape[1]
        d.counter = decode["counter"].data_ptr()
        out = decode.get("out_tokens")
        if out is not None:
            assert out.dtype == torch.int64 and out.is_contiguous() and out.shape[0] == n
            d.out_tokens, d.out_len, d.out_base = out.data_ptr(), out.shape[1], int(decode["out_base"])
        given = decode.get("given")
        if given is not None and given.dim() == 2:
            stride = given.stride(0) if n > 1 else given.shape[1]         # (one row: its stride is never applied)
            if (given.dtype != torch.int64 or given.stride(1) != 1 or given.shape[0] != n or given.shape[1] < d.capacity
                    or stride < given.shape[1] or given.device != dev):
                raise ValueError(f"given: want an int64 tensor [{n}, >= {d.capacity}] with a contiguous last dimension on {dev}, "
                                 f"got {tuple(given.shape)}")
            d.given, d.given_stride = given.data_ptr(), stride
        elif given is not None:
            if given.dtype != torch.int64 or not given.is_contiguous() or given.numel() < d.capacity or given.device != dev:
                raise ValueError(f"given: want a contiguous int64 tensor of >= {d.capacity} elements on {dev}")
            d.given = given.data_ptr()
    elif isinstance(offset, torch.Tensor):
        d.counter = _counter(dev).data_ptr()
    L.check(L.lib().cogv_sample_logits(C.byref(d), _stream()), "cogv_sample_logits")
    return ids, logp, pr


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------ candidate scoring
def score_targets(logits, targets, allow=None, group=1, logp=None, scores=None):
    """log p(target) per row of `logits` ([rows, vocab] or [b, t, vocab]; fp16 / bf16 / fp32; last dim contiguous) under a
    softmax over the ids of `allow` = (lo, hi) only (default: all), and its sum over every `group` consecutive rows -- the
    tail of the reference's inverse_prompt_score (generation/sampling.py:214-230) without the fp32 copy of the logits.
    A target outside `allow` scores -inf.  The row stride is read from the tensor, so a slice of a larger logits tensor is
    scored where it lies; a 3-D slice whose batch stride is not t row strides takes one launch per batch entry (t % group
    must be 0 then).  targets: int64, one per row.  logp / scores: optional contiguous fp32 outputs ([rows] / [rows / group]).
    Returns (logp [rows], scores [rows / group])."""
    _need_gpu(logits, targets, logp, scores)
    if logits.dim() not in (2, 3):
        raise ValueError("logits: want [rows, vocab] or [b, t, vocab]")
    assert logits.stride(-1) == 1, "logits: the vocabulary dimension must be contiguous"
    v, group = logits.shape[-1], int(group)
    # The kernel takes rows ONE stride apart.  Fold the tensor into (nb batch entries sb apart) x (nt rows st apart):
    if logits.dim() == 2:
        nb, nt, sb, st = 1, logits.shape[0], 0, logits.stride(0)
    else:
        (nb, nt), (sb, st) = logits.shape[:2], logits.stride()[:2]
    if nt == 1:
        nb, nt, st = 1, nb, sb                            # [b, 1, vocab]: the batch entries are the rows
    n = nb * nt
    if n == 1:
        st = v                                            # one row: torch reports any stride for a dimension of size 1
    if nb == 1 or sb == nt * st:
        launches = [(0, 0, n)]                            # uniform stride (2-D, contiguous 3-D): one launch for all rows
    elif group > 0 and nt % group == 0:
        launches = [(i * sb, i * nt, nt) for i in range(nb)]    # a slice like big[:, 5:9, :]: one launch per batch entry, whose
    else:                                                       # nt rows hold whole groups; (element offset, first row, rows)
        raise ValueError(f"logits: a batch stride of {sb} with {nt} rows {st} apart needs t % group == 0 (or a copy)")
    dev = logits.device
    tgt = targets.reshape(-1).to(torch.int64).contiguous()
    if tgt.numel() != n:
        raise ValueError(f"targets: want {n} ids, one per row")
    ng = n // group if group > 0 else 0
    if logp is None:
        logp = torch.empty(n, dtype=torch.float32, device=dev)
    if scores is None:
        scores = torch.empty(ng, dtype=torch.float32, device=dev)
    for name, t, cnt in (("logp", logp, n), ("scores", scores, ng)):
        if t.dtype != torch.float32 or t.numel() != cnt or not t.is_contiguous():
            raise ValueError(f"{name}: want a contiguous fp32 tensor of {cnt} elements")
    lo, hi = (0, v) if allow is None else (int(allow[0]), int(allow[1]))
    d = L.ScoreDesc()
    d.dtype, d.vocab, d.row_stride, d.allow_lo, d.allow_hi, d.group = dt_code(logits), v, st, lo, hi, group
    for off, row0, rows in launches:
        d.rows = rows
        d.logits = logits.data_ptr() + off * logits.element_size()
        d.target = tgt.data_ptr() + row0 * 8
        d.logp = logp.data_ptr() + row0 * 4
        d.scores = scores.data_ptr() + (row0 // group) * 4 if group > 0 else scores.data_ptr()
        L.check(L.lib().cogv_score_targets(C.byref(d), _stream()), "cogv_score_targets")
    return logp, scores


_COUNTERS = {}


def _counter(dev):
    """A zero-initialised completion counter per device (the sampler re-zeroes it at the end of every launch)."""
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _COUNTERS:
        _COUNTERS[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return _COUNTERS[key]


# ------------------------------------------------------------------------------------------ tokenizer ingest
_PREP_TABLES = {}     # (n_in, n_out, S) -> int32 block xmin[S], count[S], k[taps][S] of the crop's outputs of one axis
_PREP_LUT = {}


def _prep_table(n_in, n_out, first, S, taps):
    """The device layout of one axis' coefficient table (cogv_image_prep_u8), cut to the S outputs from `first` on; the
    tables come from cogv_resample_coeffs and are cached per (n_in, n_out): a data set has few distinct sizes."""
    import numpy as np
    key = (n_in, n_out, S)
    blk = _PREP_TABLES.get(key)
    if blk is None:
        rc, xmin, count, k = L.resample_coeffs(n_in, n_out, taps)
        L.check(rc, "cogv_resample_coeffs")
        blk = np.concatenate((xmin[first:first + S], count[first:first + S], k[first:first + S].T.reshape(-1))).astype(np.int32)
        if len(_PREP_TABLES) >= 4096:
            _PREP_TABLES.clear()
        _PREP_TABLES[key] = blk
    return blk


def image_prep_lut(mean, std, device=None):
    """[3, 256] fp32: what ToTensor and Normalize(mean, std) make of each byte value, computed by torch in fp32 with their
    own operations ((u / 255) - mean) / std, so that indexing it equals running them."""
    key = (tuple(float(m) for m in mean), tuple(float(v) for v in std), str(device))
    lut = _PREP_LUT.get(key)
    if lut is None:
        u = torch.arange(256, dtype=torch.float32).div(255)
        m, sd = torch.tensor(key[0], dtype=torch.float32), torch.tensor(key[1], dtype=torch.float32)
        lut = u.unsqueeze(0).sub(m.unsqueeze(1)).div(sd.unsqueeze(1)).contiguous()
        if device is not None:
            lut = lut.to(device)
        _PREP_LUT[key] = lut
    return lut


def image_prep_pack(images, size):
    """The host half of image_prep: (table [B, 8] int32, coeffs int32, byte offsets, total image bytes) for a list of uint8
    HWC images -- the per-image records and the coefficient tables cogv_image_prep_u8 reads.  Needs no device; an image
    the kernel does not take raises here with cogv_image_prep_plan's code."""
    import numpy as np
    S = int(size)
    table = np.zeros((len(images), 8), dtype=np.uint32)
    blocks, at, n_ints, off = [], {}, 0, 0
    for i, im in enumerate(images):
        if im.dim() != 3 or im.shape[2] != 3 or im.dtype != torch.uint8:
            raise ValueError(f"image {i}: want a uint8 tensor [H, W, 3], got {tuple(im.shape)} {im.dtype}")
        H, W = int(im.shape[0]), int(im.shape[1])
        rc, plan = L.image_prep_plan(H, W, S)
        L.check(rc, f"cogv_image_prep_plan({H}, {W}, {S})")
        tabs = []
        for n_in, n_out, first, taps in ((W, plan["nw"], plan["left"], plan["taps_h"]), (H, plan["nh"], plan["top"], plan["taps_v"])):
            key = (n_in, n_out)
            if key not in at:
                blk = _prep_table(n_in, n_out, first, S, taps)
                at[key] = n_ints
                blocks.append(blk)
                n_ints += blk.size
            tabs.append(at[key])
        table[i] = (off & 0xffffffff, off >> 32, H, W, tabs[0], tabs[1], plan["taps_h"], plan["taps_v"])
        off += H * W * 3
    coeffs = np.concatenate(blocks) if blocks else np.zeros(0, np.int32)
    return table.view(np.int32), coeffs, off


def image_prep(images, size, mean, std, out=None, device=None):
    """transforms.Resize(size) + CenterCrop(size) + ToTensor() + Normalize(mean, std) of a list of uint8 HWC RGB images of
    any sizes (CPU or device tensors) -> [B, size, size, 4] fp32 NHWC with channel 3 zero, the encoder's input
    (data_utils/vqvae_tokenizer.py:72-82).  Host images travel in one host-to-device copy together with their table; one
    launch does the rest.  out: optional destination; device: where host images go (default: the current device)."""
    import numpy as np
    S, B = int(size), len(images)
    if B == 0:
        raise ValueError("image_prep: no images")
    on_dev = [im.device for im in images if im.is_cuda]
    dev = on_dev[0] if on_dev else torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise L.CogviewHipError("cogview_amd ops run only on an MI355X (HIP) device: there is no CPU fallback")
    table, coeffs, nbytes = image_prep_pack(images, S)
    head = (table.nbytes + coeffs.nbytes + 15) // 16 * 16
    body = (nbytes + 15) // 16 * 16
    buf = np.zeros(head + (0 if on_dev else body), dtype=np.uint8)
    buf[:table.nbytes] = table.reshape(-1).view(np.uint8)
    buf[table.nbytes:table.nbytes + coeffs.nbytes] = coeffs.view(np.uint8)
    if on_dev:
        pad = torch.zeros(body - nbytes, dtype=torch.uint8, device=dev)
        pack = torch.cat([im.to(dev).contiguous().view(-1) for im in images] + [pad])
        dbuf = torch.from_numpy(buf).to(dev)
    else:
        at = head
        for im in images:
            flat = im.contiguous().view(-1).numpy()
            buf[at:at + flat.size] = flat
            at += flat.size
        dbuf = torch.from_numpy(buf).to(dev)
        pack = dbuf[head:]
    lut = image_prep_lut(mean, std, dev)
    if out is None:
        out = torch.empty((B, S, S, 4), dtype=torch.float32, device=dev)
    elif out.shape != (B, S, S, 4) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dbuf.device:
        raise ValueError(f"out: want a contiguous fp32 tensor [{B}, {S}, {S}, 4] on {dbuf.device}")
    rc = L.lib().cogv_image_prep_u8(_p(pack), body, C.c_void_p(dbuf.data_ptr()), C.c_void_p(table.ctypes.data),
                                    C.c_void_p(dbuf.data_ptr() + table.nbytes), coeffs.size, B, S, _p(lut), _p(out), _stream())
    L.check(rc, "cogv_image_prep_u8")
    return out


def nchw3_to_nhwc4(x):
    """[b, 3, h, w] -> [b, h, w, 4] fp32, channel 3 zero: the layout the encoder's first convolution reads."""
    _need_gpu(x)
    x = x.contiguous().float()
    b, c, h, w = x.shape
    assert c == 3, "expects RGB input"
    x4 = torch.empty((b, h, w, 4), dtype=torch.float32, device=x.device)
    L.check(L.lib().cogv_nchw3_to_nhwc4_f32(_p(x), _p(x4), b, h, w, _stream()), "cogv_nchw3_to_nhwc4_f32")
    return x4


# ------------------------------------------------------------------------------------------ VQ-VAE tokenizer training
def conv_wgrad(kind, x, dy, splits=0, relu_x=0, topologies=0):
    """Weight gradient of the convolution layer `kind` (L.CONV_4X4_S2 / CONV_1X1 / CONVT_4X4_S2; with topologies=1 also
    CONV_3X3_S1) with input x [b, ih, iw, cin] and pre-activation output gradient dy [b, oh, ow, cout], both NHWC fp32, in
    the PACKED layout the forward kernel reads: [cout, taps, cin], or [4, cout, 4, cin] for the transposed convolution
    (vqvae_zc.unpack_*_weight_grad turn it into the parameter's layout).  splits: pixel-range splits, 0 = the plan's.
    relu_x=1: the gradient against max(x, 0) -- x is the PRE-ReLU input of a layer whose forward ran with relu_in.
    topologies=1 (opt-in): 3x3 layers, and 32-wide output-channel tiles where cout <= 32."""
    _need_gpu(x, dy)
    assert x.dtype == torch.float32 and dy.dtype == torch.float32 and x.dim() == 4 and dy.dim() == 4
    x, dy = x.contiguous(), dy.contiguous()
    b, ih, iw, cin = x.shape
    cout = dy.shape[3]
    d = L.ConvWgradDesc()
    d.kind, d.B, d.IH, d.IW, d.Cin, d.Cout, d.splits = kind, b, ih, iw, cin, cout, int(splits)
    d.relu_x, d.topologies = int(relu_x), int(topologies)
    plan = (C.c_int * L.CONV_WGRAD_PLAN_INTS)()
    L.check(L.lib().cogv_conv_wgrad_plan(C.byref(d), plan), f"cogv_conv_wgrad_plan(kind {kind}, {b}x{ih}x{iw}x{cin}->{cout})")
    par, taps = (4, 4) if kind == L.CONVT_4X4_S2 else (1, {L.CONV_4X4_S2: 16, L.CONV_3X3_S1: 9}.get(kind, 1))
    om = {L.CONV_4X4_S2: (ih // 2, iw // 2), L.CONVT_4X4_S2: (ih * 2, iw * 2)}.get(kind, (ih, iw))
    assert tuple(dy.shape) == (b, om[0], om[1], cout), "dy does not have the layer's output shape"
    dw = torch.empty((4, cout, taps, cin) if par == 4 else (cout, taps, cin), dtype=torch.float32, device=x.device)
    nws = L.lib().cogv_conv_wgrad_workspace_bytes(C.byref(d))
    ws = workspace("conv_wgrad", nws, x.device) if nws else None
    d.x, d.dy, d.dw = x.data_ptr(), dy.data_ptr(), dw.data_ptr()
    d.workspace, d.workspace_bytes = (ws.data_ptr(), ws.numel()) if nws else (None, 0)
    npix = b * (ih // 2) * (iw // 2) if kind == L.CONV_4X4_S2 else b * ih * iw
    with timed_launch("conv_wgrad", 2.0 * npix * par * cout * taps * cin, 4.0 * (x.numel() + dy.numel() + dw.numel() * (1 + 2 * (plan[0] > 1) * plan[0])),
                      f"kind{kind} {b}x{ih}x{iw}x{cin}->{cout} splits {plan[0]}"):
        L.check(L.lib().cogv_conv_wgrad_nhwc_f32(C.byref(d), _stream()), "cogv_conv_wgrad_nhwc_f32")
    return dw


def relu_bias_bwd(dy, act=None):
    """(dx, db) of a layer's epilogue: dx = dy * (act > 0) for the saved post-ReLU activation `act` (None: dx is dy), db[c] =
    the sum of dx over every leading dimension, fp32, fixed order."""
    _need_gpu(dy, act)
    assert dy.dtype == torch.float32 and (act is None or (act.dtype == torch.float32 and act.shape == dy.shape))
    dy = dy.contiguous()
    act = None if act is None else act.contiguous()
    c = dy.shape[-1]
    m = dy.numel() // c
    dx = None if act is None else torch.empty_like(dy)
    db = torch.empty(c, dtype=torch.float32, device=dy.device)
    nws = L.lib().cogv_relu_bias_bwd_workspace_bytes(m, c)
    ws = workspace("relu_bias_bwd", nws, dy.device)
    with timed_launch("relu_bias_bwd", 0.0, 4.0 * dy.numel() * (1 + (act is not None) + (dx is not None)), f"{m}x{c}"):
        L.check(L.lib().cogv_relu_bias_bwd_f32(_p(dy), _p(act), _p(dx), _p(db), _p(ws), ws.numel(), m, c, _stream()),
                "cogv_relu_bias_bwd_f32")
    return (dx if act is not None else dy), db


def vq_code_stats(ids, x, n_embed):
    """(count int32 [n_embed], sum fp32 [n_embed, d]) of the pixels x [m, d] under their code ids [m] (int64): how many pixels
    chose each code and the sum of their vectors, in ascending pixel order (bitwise reproducible)."""
    _need_gpu(ids, x)
    assert ids.dtype == torch.int64 and x.dtype == torch.float32 and x.dim() == 2 and ids.numel() == x.shape[0]
    ids, x = ids.contiguous().view(-1), x.contiguous()
    m, dim = x.shape
    count = torch.empty(n_embed, dtype=torch.int32, device=x.device)
    total = torch.empty((n_embed, dim), dtype=torch.float32, device=x.device)
    nws = L.lib().cogv_vq_code_stats_workspace_bytes(m, dim, n_embed)
    ws = workspace("vq_code_stats", nws, x.device)
    with timed_launch("vq_code_stats", 1.0 * m * dim, 4.0 * (2 * x.numel() + 2 * total.numel()) + 16.0 * m, f"{m}x{dim}x{n_embed}"):
        L.check(L.lib().cogv_vq_code_stats_f32(_p(ids), _p(x), _p(count), _p(total), _p(ws), ws.numel(), m, dim, n_embed, _stream()),
                "cogv_vq_code_stats_f32")
    return count, total


def vq_ema_update(count, total, cluster_size, embed_avg, embed, decay, eps):
    """The EMA codebook update of Quantize.forward_ (vqvae/vqvae_zc.py:74-83) IN PLACE on cluster_size [n_embed], embed_avg and
    embed [d, n_embed], from vq_code_stats' (count, total).  Writes through the raw pointers: the tensors' version counters do
    not move (the caller invalidates what it derived from them).  Returns n = cluster_size.sum() as a device scalar."""
    _need_gpu(count, total, cluster_size, embed_avg, embed)
    dim, n_embed = embed.shape
    for t in (cluster_size, embed_avg, embed, total):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert count.dtype == torch.int32 and tuple(total.shape) == (n_embed, dim) and embed_avg.shape == embed.shape
    n = torch.empty(1, dtype=torch.float32, device=embed.device)
    with timed_launch("vq_ema_update", 4.0 * embed.numel(), 4.0 * 4 * embed.numel(), f"{dim}x{n_embed}"):
        L.check(L.lib().cogv_vq_ema_update_f32(_p(count), _p(total), _p(cluster_size), _p(embed_avg), _p(embed), _p(n), float(decay),
                                               float(eps), dim, n_embed, _stream()), "cogv_vq_ema_update_f32")
    return n


def vq_ste_bwd(g_q, g_diff, x, q):
    """Gradient of the quantiser's input: g_q + g_diff * 2 (x - q) / numel (straight-through estimator + commitment term,
    vqvae/vqvae_zc.py:85-86).  g_q / g_diff (a device scalar) may be None."""
    _need_gpu(x, q, g_q, g_diff)
    x, q = x.contiguous(), q.contiguous()
    g_q = None if g_q is None else g_q.contiguous()
    g_x = torch.empty_like(x)
    with timed_launch("vq_ste_bwd", 3.0 * x.numel(), 4.0 * 4 * x.numel(), f"{x.numel()}"):
        L.check(L.lib().cogv_vq_ste_bwd_f32(_p(g_q), _p(g_diff), _p(x), _p(q), _p(g_x), x.numel(), _stream()), "cogv_vq_ste_bwd_f32")
    return g_x


def sr_patches(x4, positions):
    """The device half of make_super_resolution_batch (preprocess/pretokenized_data.py:100-124) on x4 [b, S, S, 4] fp32:
    (patches [b * k, S/2, S/2, 4], image-major, patch i * k + j = image i at crop positions[j] in 0..8 of the 3 x 3 grid
    with step S/4; overview [b, S/2, S/2, 4] = F.interpolate(size=(S/2, S/2), mode='bilinear')).  positions: a list or an
    int tensor on either side, shared by all images."""
    _need_gpu(x4)
    if x4.dim() != 4 or x4.shape[3] != 4 or x4.shape[1] != x4.shape[2] or x4.dtype != torch.float32:
        raise ValueError(f"x4: want an fp32 tensor [b, S, S, 4], got {tuple(x4.shape)} {x4.dtype}")
    pos = [int(v) for v in (positions.reshape(-1).tolist() if isinstance(positions, torch.Tensor) else positions)]
    if not pos or any(v < 0 or v > 8 for v in pos):
        raise ValueError(f"positions: want one or more of 0..8, got {pos}")
    x4 = x4.contiguous()
    b, S, k = x4.shape[0], x4.shape[1], len(pos)
    pos_t = torch.tensor(pos, dtype=torch.int32, device=x4.device)
    patches = torch.empty((b * k, S // 2, S // 2, 4), dtype=torch.float32, device=x4.device)
    overview = torch.empty((b, S // 2, S // 2, 4), dtype=torch.float32, device=x4.device)
    L.check(L.lib().cogv_sr_patches_nhwc4_f32(_p(x4), _p(pos_t), _p(patches), _p(overview), b, S, k, _stream()),
            "cogv_sr_patches_nhwc4_f32")
    return patches, overview


# ------------------------------------------------------------------------------------------ image egress
_GRID_TABLES = {}     # (device, table bytes) -> the source table on the device; the key IS the content
_GRID_TABLES_CAPTURED = {}     # the tables among them that a stream capture has recorded


def image_grid_sources(images, size=None):
    """The host half of image_grid: (sources, table [K, 8] int32, B, H, W) for a tensor [B, 3, h, w] / [3, h, w] or a list
    of such tensors of different sizes.  size=(H, W): the size every image is replicated to by an integer factor (default:
    the largest source).  The table holds the sources' device pointers, so the returned sources must outlive its use."""
    import numpy as np
    srcs = [images] if isinstance(images, torch.Tensor) else list(images)
    if not srcs:
        raise ValueError("image_grid: no images")
    _need_gpu(*srcs)
    srcs = [s.unsqueeze(0) if s.dim() == 3 else s for s in srcs]
    for s in srcs:
        if s.dim() != 4 or s.shape[1] != 3 or s.dtype != torch.float32:
            raise ValueError(f"image_grid: want fp32 tensors [B, 3, H, W] or [3, H, W], got {tuple(s.shape)} {s.dtype}")
    srcs = [s.contiguous() for s in srcs if s.shape[0] > 0]
    if not srcs:
        raise ValueError("image_grid: no images")
    if size is None:
        H, W = max(int(s.shape[2]) for s in srcs), max(int(s.shape[3]) for s in srcs)
    else:
        H, W = int(size[0]), int(size[1])
    table = np.zeros((len(srcs), 8), dtype=np.uint32)
    first = 0
    for k, s in enumerate(srcs):
        n, h, w = int(s.shape[0]), int(s.shape[2]), int(s.shape[3])
        ptr = s.data_ptr()
        table[k] = (ptr & 0xffffffff, ptr >> 32, n, h, w, H // h if h <= H else 0, first, 0)
        first += n
    return srcs, table.view(np.int32), first, H, W


def image_grid(images, nrow=8, padding=2, normalize=False, value_range=None, scale_each=False, pad_value=0.0, size=None,
               out=None):
    """torchvision.utils.make_grid followed by save_image's conversion (mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0)
    .to(uint8)) on the device, byte for byte as torch computes them on CPU tensors (generate_samples.py:175-199, :236-244,
    preprocess/utils.py:25-31) -> uint8 [GH, GW, 3].  images: a CUDA fp32 tensor [B, 3, H, W] or [3, H, W], or a list of such
    tensors of different sizes; size=(H, W) (default: the largest) is what each is brought to by nearest replication with an
    integer factor 1, 2, 4 or 8 (F.interpolate(size=...) at these factors).  Nothing is read back: with normalize and no
    value_range the extremes stay in device memory between the two launches.  out: optional uint8 destination of exactly
    GH * GW * 3 elements, 16-byte aligned."""
    srcs, table, B, H, W = image_grid_sources(images, size)
    dev = srcs[0].device
    nrow, padding = int(nrow), int(padding)
    if value_range is not None and not isinstance(value_range, tuple):
        raise TypeError("value_range has to be a tuple (min, max) if specified. min and max are numbers")
    each = bool(normalize and scale_each and value_range is None)
    rc, plan = L.image_grid_plan(B, H, W, nrow, padding, each, table)
    L.check(rc, f"cogv_image_grid_plan({B}, {H}, {W}, nrow={nrow}, padding={padding})")
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), table.tobytes())
    dtab = _GRID_TABLES_CAPTURED.get(key, _GRID_TABLES.get(key))
    if dtab is None:
        if len(_GRID_TABLES) >= 256:
            _GRID_TABLES.clear()
        dtab = _GRID_TABLES[key] = torch.from_numpy(table.copy()).to(dev)
    if torch.cuda.is_current_stream_capturing():
        _GRID_TABLES_CAPTURED[key] = dtab      # a captured graph reads this table at every replay: never dropped
    K, src_bytes = table.shape[0], 4 * sum(s.numel() for s in srcs)
    shape = (plan["grid_h"], plan["grid_w"], 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif out.numel() != plan["out_bytes"] or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out: want a contiguous uint8 tensor of {list(shape)} on {dev}")
    mode, rng, low, high = L.GRID_NORM_NONE, None, 0.0, 0.0
    if normalize and value_range is not None:
        mode, low, high = L.GRID_NORM_FIXED, float(value_range[0]), float(value_range[1])
    elif normalize:
        mode = L.GRID_NORM_RANGE_EACH if each else L.GRID_NORM_RANGE
        rng = torch.empty(plan["range_bytes"] // 4, dtype=torch.int32, device=dev)
        with timed_launch("image_range", 0.0, src_bytes, lambda: f"{B}x3x{H}x{W}" + (" per image" if each else "")):
            rc = L.lib().cogv_image_range_f32(_p(dtab), C.c_void_p(table.ctypes.data), K, B, H, W, int(each), _p(rng),
                                              plan["range_bytes"], _stream())
        L.check(rc, "cogv_image_range_f32")
    with timed_launch("image_grid", 0.0, src_bytes + plan["out_bytes"], lambda: f"{B}x3x{H}x{W} -> {shape[0]}x{shape[1]}x3"):
        rc = L.lib().cogv_image_grid_u8(_p(dtab), C.c_void_p(table.ctypes.data), K, B, H, W, nrow, padding, float(pad_value), mode,
                                        _p(rng), low, high, _p(out), plan["out_bytes"], _stream())
    L.check(rc, "cogv_image_grid_u8")
    return out.view(shape)
