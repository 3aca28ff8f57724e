"""GPU: every cell of the skinny-M launch plan (csrc/gemv_plan.h) executed -- tests/gemv_cells.py holds the grid, and
tests/test_gemv_plan.py proves on the CPU that the grid reaches every plan entry of every kind, format and dtype.
Per cell: (a) an exact-integer product, bit-equal to fp64; (b) a `randn` product against fp64 element by element;
(c) LayerNorm kind: the criterion of test_gemv_with_layernorm_prologue; (d) a second call gives the same bits.
Beside the sweep: (e) 17 and 32 key splits through both combines, (f) leading dimensions with canaries around every output,
(g) the first generation alone (COGV_GEMV2=0) in a fresh process.

Worst err / bound of (b) as measured: DESIGN.md 4.5.1."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from oracle import cogview_oracle as O
from tests import gemv_cells as GC
from tests.test_kernels_gpu import TOL, rel
from tests.test_w8_gemv_gpu import TOL_LN, dequant

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = [(kind, w8, dtype) for w8 in GC.FORMATS for kind in GC.KINDS for dtype in GC.DTYPES]
IDS = [f"{'e4m3' if w8 else 'w16'}-{kind}-{GC.DT_NAME[dtype]}" for kind, w8, dtype in CELLS]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("kind,w8,dtype", CELLS, ids=IDS)
def test_exact_integer_product(ops, kind, w8, dtype):
    """(a), (d): x, W in {-1, 0, 1}, integer bias (E4M3: bytes 0x38 / 0xB8 / 0x00 with scale 1, then a power of two per row;
    attn: synthesised partials at 1 and 32 splits; ln: gamma = 0, beta = x, plain-input and post-LN form) == fp64, to the bit."""
    fails, ran, refused = GC.exact_sweep(ops, kind, w8, dtype)
    print(f"{kind} w8={w8} {dtype}: {ran} cells launched, {refused} refused by the plan, {len(fails)} failures")
    assert not fails, "\n".join(fails[:40])
    assert ran + refused == len(GC.ks(kind)) * len(GC.MS) * len(GC.NS) and (refused == 0 or w8)


def _randn_operands(ops, kind, w8, dtype, K):
    """x [8, K], the weight as the kernels see it in fp64 [136, K], bias, and the Product that launches them"""
    g = torch.Generator().manual_seed(7 * K + 1)
    x = torch.randn((GC.M_MAX, K), generator=g)
    if kind != "attn":
        x = x.to(dtype).float()                      # plain, ln: x is stored in the 16-bit type; attn: rounded inside the kernel
    w = (torch.randn((GC.N_MAX, K), generator=g) * 0.05).to(dtype)
    bias = torch.randn(GC.N_MAX, generator=g).to(dtype)
    qs = ops.quantize_rows_e4m3(w.cuda()) if w8 else None
    weff = dequant(qs) if w8 else w.double()
    prod = GC.Product(ops, kind, w8, dtype, K, x, w, bias, qs=qs, z=torch.randn((GC.M_MAX, K), generator=g) * 3.0)
    if kind == "ln":
        x = x[:1].expand(GC.M_MAX, K)
    return x.double(), weff, bias.double(), prod


def _ln_composition(ops, prod, w8, dtype, K, M, N, post, gelu, stream32, g):
    """(c) on one cell: the Sandwich-LN launches followed by the plain product of the same library"""
    dev = "cuda"
    z = (torch.randn((M, K), generator=g) * 3.0).to(torch.float32 if (stream32 and not post) else dtype).to(dev)
    res = torch.randn((M, K), generator=g).to(torch.float32 if stream32 else dtype).to(dev)
    gp, bp, gn, bn = [(o + 0.1 * torch.randn(K, generator=g)).to(dtype).to(dev) for o in (1.0, 0.0, 1.0, 0.0)]
    w, bias = prod.weight(N), prod.bias[:N]
    gemm = (lambda a, **kw: ops.gemm_w8(a, w, **kw)) if w8 else (lambda a, **kw: ops.gemm(a, w, **kw))
    fused = ops.gemv_ln_w8 if w8 else ops.gemv_ln
    zmax = ops.absmax(z)
    if post:
        slot_t = ops.new_absmax_slot(z.device)
        t_ref, _, _ = ops.sandwich_ln_fwd(z, gp, bp, GC.EPS, zmax, residual=res, absmax_out=slot_t, save_stats=False)
    else:
        t_ref, slot_t = z, zmax
    x_ref, _, _ = ops.sandwich_ln_fwd(t_ref, gn, bn, GC.EPS, slot_t, save_stats=False)
    out_ref = gemm(x_ref, bias=bias, gelu=gelu)
    kw = dict(post=(gp, bp), residual=res, want_t=True) if post else {}
    out, t = fused(z, w, bias, gn, bn, GC.EPS, z_absmax=zmax, gelu=gelu, **kw)
    bad = []
    if post:
        # (all-16-bit stream: t against the Sandwich-LN kernel's bits is test_layernorm_prologue_residual_stream_bits)
        if stream32 and (t.dtype != torch.float32 or rel(t, t_ref) >= 1e-6):
            bad.append("t (fp32 stream)")
        out2, t2 = fused(z, w, bias, gn, bn, GC.EPS, z_absmax=None, gelu=gelu, **kw)
        if not (torch.equal(out2, out) and torch.equal(t2, t)):
            bad.append("z_absmax=None differs from the published scalar")
    e = rel(out, out_ref)
    if not e < TOL_LN[dtype]:
        bad.append(f"against the composition {e:.2e}")
    weff = dequant(w) if w8 else w.double().cpu()
    ref = x_ref.double().cpu() @ weff.t() + bias.double().cpu()
    if gelu:
        ref = O.gelu(ref.to(dtype).float())
    e = rel(out, ref)
    if not e < TOL[dtype]:
        bad.append(f"against fp64 of the composition's x_in {e:.2e}")
    return bad


@pytest.mark.parametrize("kind,w8,dtype", CELLS, ids=IDS)
def test_randn_product(ops, kind, w8, dtype):
    """(b): |got - ref| <= bound (tests/gemv_cells.py: bound) element by element on the bias-only output, GeLU outputs within the
    relative-L2 bar TOL; (c) on every cell of the LayerNorm kind, the fp32-stream form at one K per class."""
    fails, worst = [], {}
    for K in GC.ks(kind):
        x, weff, bias, prod = _randn_operands(ops, kind, w8, dtype, K)
        absdot = x.abs() @ weff.abs().t()
        ref = x @ weff.t() + bias
        bnd = GC.bound(ref, absdot, bias, K, dtype, x_rounded=kind == "attn").cuda()
        ref_d, gelu_ref = ref.cuda(), O.gelu(ref.float())
        g = torch.Generator().manual_seed(K + 5)
        for M in GC.MS:
            for N in GC.NS:
                rc, out = GC.plan(kind, w8, dtype, M, N, K)
                if rc != 0:
                    continue
                form = GC.form_name(out)
                where = f"M={M} N={N} K={K} [{form}]"
                got = prod(M, N)
                ratio = float(((got.double() - ref_d[:M, :N]).abs() / bnd[:M, :N]).max())
                worst[form] = max(worst.get(form, 0.0), ratio)
                if not ratio <= GC.BOUND_FACTOR[form]:
                    fails.append(f"{where}: err / bound = {ratio:.3f}")
                if kind != "attn":
                    e = rel(prod(M, N, gelu=True), gelu_ref[:M, :N])
                    if not e < TOL[dtype]:
                        fails.append(f"{where}: GeLU output rel-L2 {e:.2e}")
                if kind == "ln":
                    gelu = bool((M + N // 8 + K // 512) & 1)
                    modes = [(True, False), (False, False)] + ([(True, True), (False, True)] if K in GC.LN_STREAM32_KS and N == 40 else [])
                    for post, stream32 in modes:
                        fails += [f"{where} post={post} gelu={gelu} stream32={stream32}: {b}"
                                  for b in _ln_composition(ops, prod, w8, dtype, K, M, N, post, gelu, stream32, g)]
    for form, r in sorted(worst.items()):
        print(f"RATIO {'e4m3' if w8 else 'w16'} {form} {kind} {GC.DT_NAME[dtype]}: worst err / bound = {r:.4f}")
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("dtype", GC.DTYPES, ids=GC.DT_NAME.get)
@pytest.mark.parametrize("w8", GC.FORMATS, ids=["w16", "e4m3"])
def test_layernorm_prologue_residual_stream_bits(ops, dtype, w8):
    """(c), first criterion, on every cell of the LayerNorm kind: t = residual + LN_post(z) as workgroup 0 writes it is bit-equal
    to the Sandwich-LN kernel's (all-16-bit stream; `randn` z * 3, residual, gamma = 1 + 0.1 randn, beta = 0.1 randn).

    This sweep found the one defect of the pull request that added it: with the statistics of the post-LayerNorm summed over the
    4 or 8 waves of the prologue (chains of K / 256 or K / 512 elements per lane, a wave sum each, a pairwise sum over the
    waves) where ln_fwd_kernel gives a row to ONE wave (chains of K / 64, one wave sum), the fp32 mean and variance differed in
    their last bits and now and then moved a rounding: on 16-bit weights 12 of the 126 cells (fp16) and 1 of 126 (bf16), on
    E4M3 weights 10 and 1 of 114, 1 to 3 elements of t each, at every K from 1024 up, in V, M and first-generation plans.  The
    prologues now take these statistics one wave per row, in ln_fwd_kernel's order and with its roundings spelled out
    (common.cuh: ln_row_stats_wave; the order alone left 3 cells of 126, where the compiler had fused a multiply-add in one
    kernel and not in the other)."""
    fused = ops.gemv_ln_w8 if w8 else ops.gemv_ln
    cells, bad, worst = 0, [], 0
    for K in GC.ks("ln"):
        g = torch.Generator().manual_seed(3 * K + 2)
        w = (torch.randn((GC.N_MAX, K), generator=g) * 0.05).to(dtype).cuda()
        qs, bias = ops.quantize_rows_e4m3(w), torch.randn(GC.N_MAX, generator=g).to(dtype).cuda()
        for M in GC.MS:
            for N in GC.NS:
                rc, out = GC.plan("ln", w8, dtype, M, N, K)
                if rc != 0:
                    continue
                cells += 1
                z, res = [(torch.randn((M, K), generator=g) * s).to(dtype).cuda() for s in (3.0, 1.0)]
                gp, bp, gn, bn = [(o + 0.1 * torch.randn(K, generator=g)).to(dtype).cuda() for o in (1.0, 0.0, 1.0, 0.0)]
                zmax = ops.absmax(z)
                t_ref, _, _ = ops.sandwich_ln_fwd(z, gp, bp, GC.EPS, zmax, residual=res, save_stats=False)
                _, t = fused(z, (qs[0][:N], qs[1][:N]) if w8 else w[:N], bias[:N], gn, bn, GC.EPS, z_absmax=zmax, post=(gp, bp),
                             residual=res, want_t=True)
                if not torch.equal(t, t_ref):
                    ulps = int((t.view(torch.int16).int() - t_ref.view(torch.int16).int()).abs().max())
                    worst = max(worst, ulps)
                    bad.append(f"M={M} N={N} K={K} [{GC.form_name(out)}]: {int((t != t_ref).sum())} of {t.numel()} elements, <= {ulps} ulp")
    print(f"TBITS {'e4m3' if w8 else 'w16'} {GC.DT_NAME[dtype]}: {len(bad)} of {cells} cells differ, worst {worst} ulp")
    assert not bad, "\n".join(bad[:40])


# ------------------------------------------------------------------------------------------------------------ (e) key splits
@pytest.mark.parametrize("dtype", GC.DTYPES, ids=GC.DT_NAME.get)
@pytest.mark.parametrize("kv8", [False, True], ids=["kv16", "kv8"])
def test_seventeen_and_thirty_two_key_splits(ops, dtype, kv8):
    """Capacities 2176 and 4096: attn_decode_combine_kernel's branch for more than 16 splits against the oracle, and the
    combine prologues (16-bit and E4M3 weights) bit-equal to combine + plain product -- also with `first` set so that whole
    splits are empty (m = -inf)."""
    from tests.test_kv8_kernels_gpu import cpu_quantize, dequantize, heads_of
    from tests.test_ragged_decode_kernels_gpu import _first, _reference
    H, N = 8, 136
    hp = H * 64
    firsts = [300, 0, 129, 2047, 1000, 5, 128, 2000]
    g = torch.Generator().manual_seed(17 + 32)
    # one cache for all shapes (smaller ones take its leading rows and slots); kept as the fp32 values the kernels see
    cache = torch.randn((8, 4096, 2 * hp), generator=g).to(dtype)
    if kv8:
        q0, s0 = cpu_quantize(heads_of(cache, H))
        seen = dequantize(q0, s0)
    else:
        seen = cache.float()
    w, bias = (torch.randn((N, hp), generator=g) * 0.05).to(dtype).cuda(), torch.randn(N, generator=g).to(dtype).cuda()
    qs = ops.quantize_rows_e4m3(w)
    for cap in (2176, 4096):
        for b in (1, 2, 8):
            for pos in (cap - 1, 2048):
                qkv = (torch.randn((b, 1, 3 * hp), generator=g)).to(dtype)
                pos_d = torch.tensor([pos], dtype=torch.int64, device="cuda")
                for first in (None, firsts[:b]):
                    first_d = None if first is None else _first(first)
                    if kv8:
                        store = (q0[:b, :, :, :cap].contiguous().cuda(), s0[:b, :, :, :cap].contiguous().cuda())
                        run = lambda **kw: ops.attention_decode_kv8(qkv.cuda(), store, pos_d, H, first=first_d, **kw)
                    else:
                        store = cache[:b, :cap].contiguous().cuda()
                        run = lambda **kw: ops.attention_decode(qkv.cuda(), store, pos_d, H, first=first_d, **kw)
                    att = run()
                    # the slots as the kernel left them: slot pos holds the new token's key | value
                    if kv8:
                        new = dequantize(store[0][:, :, :, pos:pos + 1].cpu(), store[1][:, :, :, pos:pos + 1].cpu())[:, 0]
                    else:
                        new = store[:, pos].cpu().float()
                    assert torch.equal(store[:, pos].cpu(), qkv[:, 0, hp:]) if not kv8 else bool(torch.isfinite(new).all())
                    kv = seen[:b, :pos + 1].clone()
                    kv[:, pos] = new
                    e = rel(att, _reference(qkv, kv, H, pos, first or [0] * b))
                    where = f"cap={cap} b={b} pos={pos} first={first}"
                    assert e < TOL[dtype], (where, e)
                    two, two8 = ops.gemm(att.view(b, hp), w, bias=bias), ops.gemm_w8(att.view(b, hp), qs, bias=bias)
                    parts = run(combine=False)
                    assert torch.equal(ops.gemv_attn(parts, b, H, cap, w, bias=bias), two), where
                    assert torch.equal(ops.gemv_attn_w8(parts, b, H, cap, qs, dtype, bias=bias), two8), where


# ------------------------------------------------------------------------------------------------------------ (f) leading dimensions
SENTINEL = 0x7BCD                                     # a finite 16-bit pattern in either type; no kernel output here equals it
# one cell per form: V, M, two halves, first generation (16-bit only)
LD_CELLS = [(False, 1, 1024, "V"), (False, 3, 1536, "M"), (False, 8, 10240, "M-k2"), (False, 5, 5632, "gen1"),
            (True, 1, 2560, "V"), (True, 3, 3072, "M"), (True, 8, 4096, "M-k2"), (True, 4, 10240, "M-k2")]


def _canary(M, N, dtype):
    buf = torch.full((8, N + 24), SENTINEL, dtype=torch.int16, device="cuda")
    return buf, buf.view(dtype)[:M, :N]


def _intact(buf, M, N):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:M, :N] = False
    return bool((buf[mask] == SENTINEL).all())


@pytest.mark.parametrize("dtype", GC.DTYPES, ids=GC.DT_NAME.get)
@pytest.mark.parametrize("w8,M,K,form", LD_CELLS)
def test_leading_dimensions_and_canaries(ops, dtype, w8, M, K, form):
    """x with lda = K + 8, W / q with ldb = K + 16 (padding: NaN), the output (and the GeLU pre-activation) the leading [M, N] of
    an [8, N + 24] buffer of sentinels: the bits of the contiguous call, and every sentinel intact -- the MFMA forms compute
    padding rows m >= M, and a store there or past column N would land in a neighbour."""
    from cogview_amd import _lib
    N = 40
    rc, out = GC.plan("plain", w8, dtype, M, N, K)
    assert rc == 0 and GC.form_name(out) == form
    g = torch.Generator().manual_seed(K + M)
    x = torch.randn((M, K), generator=g).to(dtype).cuda()
    w = (torch.randn((N, K), generator=g) * 0.05).to(dtype).cuda()
    bias = torch.randn(N, generator=g).to(dtype).cuda()
    xs = torch.full((8, K + 8), float("nan"), dtype=dtype, device="cuda")
    xs[:M, :K] = x
    xv = xs[:M, :K]
    buf, outv = _canary(M, N, dtype)
    if w8:
        q, scale = ops.quantize_rows_e4m3(w)
        qb = torch.full((N, K + 16), 0x7F, dtype=torch.uint8, device="cuda")          # 0x7F: NaN
        qb[:, :K] = q
        want = ops.gemm_w8(x, (q, scale), bias=bias)
        d, wq, _ = ops._w8_call(dtype, M, K, (qb[:, :K], scale), bias, False, None)
        d.A, d.lda, d.C, d.ldc = xv.data_ptr(), xv.stride(0), outv.data_ptr(), outv.stride(0)
        assert wq.ldq == K + 16 and d.lda == K + 8 and d.ldc == N + 24
        _lib.check(_lib.lib().cogv_gemm_w8(C.byref(d), C.byref(wq), ops._stream()), "cogv_gemm_w8")
    else:
        wb = torch.full((N, K + 16), float("nan"), dtype=dtype, device="cuda")
        wb[:, :K] = w
        want = ops.gemm(x, w, bias=bias)
        ops.gemm(xv, wb[:, :K], bias=bias, out=outv)
    assert bool(torch.isfinite(want.float()).all())
    assert torch.equal(outv, want) and _intact(buf, M, N)
    if not w8:                                        # the GeLU pre-activation travels through ldaux
        aux_want = torch.empty_like(want)
        act_want = ops.gemm(x, w, bias=bias, gelu=True, gelu_aux=aux_want)
        assert torch.equal(aux_want, want)
        buf2, outv2 = _canary(M, N, dtype)
        abuf, auxv = _canary(M, N, dtype)
        ops.gemm(xv, wb[:, :K], bias=bias, gelu=True, gelu_aux=auxv, out=outv2)
        assert torch.equal(outv2, act_want) and torch.equal(auxv, aux_want) and _intact(buf2, M, N) and _intact(abuf, M, N)


# V | M, one tile | M, 8 waves at the largest LDS it takes | first generation, 64 KB by attribute | the E4M3 forms: V, 2 and 4 tiles
LN_CANARY_CELLS = [(False, 1, 1024), (False, 3, 1536), (False, 8, 3072), (False, 8, 4096), (True, 1, 2560), (True, 2, 512), (True, 5, 3072)]


@pytest.mark.parametrize("dtype", GC.DTYPES, ids=GC.DT_NAME.get)
@pytest.mark.parametrize("w8,M,K", LN_CANARY_CELLS)
def test_residual_stream_canary(ops, dtype, w8, M, K):
    """LayerNorm kind: t_out points into a flat buffer of sentinels (ops allocates t itself, so the descriptor is filled here):
    the M rows are those of the ordinary call, and nothing in front of them or behind them -- where the padding rows m >= M of
    the row bucket would land -- is written."""
    from cogview_amd import _lib
    N, guard = 40, 64
    g = torch.Generator().manual_seed(K + M)
    z, res = [(torch.randn((M, K), generator=g) * s).to(dtype).cuda() for s in (3.0, 1.0)]
    gp, bp, gn, bn = [(o + 0.1 * torch.randn(K, generator=g)).to(dtype).cuda() for o in (1.0, 0.0, 1.0, 0.0)]
    w, bias = (torch.randn((N, K), generator=g) * 0.05).to(dtype).cuda(), torch.randn(N, generator=g).to(dtype).cuda()
    qs = ops.quantize_rows_e4m3(w)
    want, want_t = (ops.gemv_ln_w8 if w8 else ops.gemv_ln)(z, qs if w8 else w, bias, gn, bn, GC.EPS, post=(gp, bp), residual=res, want_t=True)
    flat = torch.full((guard + 8 * K + guard,), SENTINEL, dtype=torch.int16, device="cuda")
    ln, _ = ops._ln_prologue(z, gn, bn, GC.EPS, None, (gp, bp), res, True)
    ln.t_out = flat.data_ptr() + 2 * guard
    if w8:
        d, wq, out = ops._w8_call(dtype, M, K, qs, bias, False, None)
        _lib.check(_lib.lib().cogv_gemv_ln_w8(C.byref(d), C.byref(ln), C.byref(wq), ops._stream()), "cogv_gemv_ln_w8")
    else:
        out = torch.empty((M, N), dtype=dtype, device="cuda")
        d = ops._skinny_desc(out, K, bias, False, None)
        d.A, d.B, d.ldb = z.data_ptr(), w.data_ptr(), K
        _lib.check(_lib.lib().cogv_gemv_ln(C.byref(d), C.byref(ln), ops._stream()), "cogv_gemv_ln")
    assert torch.equal(out, want)
    assert torch.equal(flat[guard:guard + M * K].view(dtype).view(M, K), want_t)
    assert bool((flat[:guard] == SENTINEL).all()) and bool((flat[guard + M * K:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------ (g) COGV_GEMV2=0
def test_first_generation_alone():
    """COGV_GEMV2=0 is read once per process: a fresh child runs the 16-bit exact-integer sweep of all three kinds on the first
    generation's three kernels and prints one line per failure."""
    r = subprocess.run([sys.executable, "-m", "tests.gemv_cells"], cwd=ROOT, env=dict(os.environ, COGV_GEMV2="0"),
                       capture_output=True, text=True, timeout=300)
    lines = r.stdout.splitlines()
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert not [l for l in lines if l.startswith("FAIL")], "\n".join(l for l in lines if l.startswith("FAIL"))[:4000]
    gens = [l for l in lines if l.startswith("generations")]
    assert len(gens) == 6 and all(l.endswith(": [1]") for l in gens), gens
    n = sum(len(GC.ks(kind)) for kind in GC.KINDS) * len(GC.MS) * len(GC.NS) * 2
    assert f"cells {n}" in lines
