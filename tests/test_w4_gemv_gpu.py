"""GPU: the skinny-M products on a 4-bit (OCP MXFP4) weight operand -- cogv_gemm_w4, cogv_gemv_ln_w4, cogv_gemv_attn_w4 through
ops -- on every cell of the 4-bit launch plans (tests/w4_cases.py holds the grid; tests/test_w4_cpu.py proves that it reaches every
plan).  Per cell: (a) an exact-integer product, bit-equal to fp64; (b) a `randn` product against fp64 on the dequantized weights,
element by element, by the bound of tests/gemv_cells.py; a second call gives the same bits.  Beside the sweep: the
combine-prologue form against the two-launch form, the LayerNorm form against its composition at the cases and bars of
tests/test_w8_gemv_gpu.py, strided operands inside sentinel buffers, unsupported shapes.

Worst err / bound of (b) as measured: DESIGN.md 4.5.7."""
import pytest
import torch

from oracle import cogview_oracle as O
from tests import gemv_cells as GC
from tests import w4_cases as W4
from tests.test_w8_gemv_gpu import TOL, TOL_LN, rel, rnd

pytestmark = pytest.mark.gpu

CELLS = [(kind, dtype) for kind in W4.KINDS for dtype in W4.DTYPES]
IDS = [f"{kind}-{GC.DT_NAME[dtype]}" for kind, dtype in CELLS]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("kind,dtype", CELLS, ids=IDS)
def test_exact_integer_product(ops, kind, dtype):
    """(a): codes in {-1, 0, 1}, a block scale of {1, 2, 1/2} per 32 elements (a misplaced scale byte changes a multiple of 1/2), x
    in {-1, 0, 1}, integer bias; attn: synthesised partials at 1 and 32 splits; ln: gamma = 0, beta = x, plain-input and post-LN
    form.  Every partial sum is a multiple of 1/2 far below 2^24: the result equals fp64 to the bit in every class."""
    fails, ran, refused = [], 0, 0
    for K in W4.ks(kind):
        x, qs, w, bias, dot = W4.exact_operands(K, dtype)
        g = torch.Generator().manual_seed(K + 1)
        prod = W4.Product(ops, kind, dtype, K, x, qs, bias, z=torch.randn((W4.M_MAX, K), generator=g))
        if kind == "ln":
            dot = dot[:1].expand(W4.M_MAX, W4.N_MAX)
        ref = dot + bias
        ref_d, nobias_d = ref.to(dtype).cuda(), dot.to(dtype).cuda()
        assert torch.equal(ref_d.double().cpu(), ref)
        for M in W4.MS:
            for N in W4.NS:
                rc, out = W4.plan(kind, dtype, M, N, K, nsplit=32 if kind == "attn" else 1)
                where = f"{kind} {GC.DT_NAME[dtype]} M={M} N={N} K={K}"
                if rc != 0:
                    refused += 1
                    try:
                        prod(M, N)
                        fails.append(f"{where}: the plan refuses ({rc}) but the call launched")
                    except Exception as e:
                        if "unsupported" not in str(e):
                            fails.append(f"{where}: {e}")
                    continue
                ran += 1
                where += f" [{GC.form_name(out)}]"
                variants = [dict(cap=cap) for cap in W4.CAPS] if kind == "attn" else [dict(), dict(post=True)] if kind == "ln" else [dict()]
                for kw in variants:
                    got = prod(M, N, **kw)
                    if got is None:
                        fails.append(f"{where} {kw}: t is not beta_post")
                    elif got.shape != (M, N) or got.dtype != dtype or not torch.equal(got, ref_d[:M, :N]):
                        fails.append(f"{where} {kw}: {int((got != ref_d[:M, :N]).sum())} wrong elements")
                    elif not torch.equal(prod(M, N, **kw), got):
                        fails.append(f"{where} {kw}: the second call gives other bits")
                got = prod(M, N, bias=False)
                if not torch.equal(got, nobias_d[:M, :N]):
                    fails.append(f"{where} no bias: {int((got != nobias_d[:M, :N]).sum())} wrong elements")
    print(f"{kind} {dtype}: {ran} cells launched, {refused} refused by the plan, {len(fails)} failures")
    assert not fails, "\n".join(fails[:40])
    assert ran + refused == len(W4.ks(kind)) * len(W4.MS) * len(W4.NS) and ran > refused


_RANDN = {}


def _randn_weights(ops, dtype, K):
    """weights of standard deviation 0.02 through the device quantizer (shared by the kinds): (q, s) on the CPU, their values in fp64"""
    if (dtype, K) not in _RANDN:
        g = torch.Generator().manual_seed(7 * K + 1)
        w = (torch.randn((W4.N_MAX, K), generator=g) * 0.02).to(dtype)
        q, s = (t.cpu() for t in ops.quantize_rows_mxfp4(w.cuda()))
        weff = W4.dequantize(q, s)
        # the kernels convert a code with its block scale folded in, to fp32 (one row) or to the storage type (more rows): the values
        # must be exact there -- in fp16 that is the condition of the issue (multiples of 2^-24 below 65520)
        assert torch.equal(weff.to(dtype).double(), weff), "the dequantized weights are not exact in the storage type"
        assert torch.equal(weff.float().double(), weff)
        _RANDN[(dtype, K)] = (q, s, weff)
    return _RANDN[(dtype, K)]


@pytest.mark.parametrize("kind,dtype", CELLS, ids=IDS)
def test_randn_product(ops, kind, dtype):
    """(b): |got - ref| <= u |ref| + 2 K 2^-24 (|x| |W_dq|^T + |bias|) + 2^-24 (+ u |x| |W_dq|^T for the attention kind) element by
    element, ref in fp64 on the dequantized weights; GeLU outputs within the relative-L2 bar of tests/test_w8_gemv_gpu.py."""
    fails, worst = [], {}
    for K in W4.ks(kind):
        q, s, weff = _randn_weights(ops, dtype, K)
        g = torch.Generator().manual_seed(11 * K + 3)
        x = torch.randn((W4.M_MAX, K), generator=g)
        if kind != "attn":
            x = x.to(dtype).float()
        bias = torch.randn(W4.N_MAX, generator=g).to(dtype)
        prod = W4.Product(ops, kind, dtype, K, x, (q, s), bias, z=torch.randn((W4.M_MAX, K), generator=g) * 3.0)
        if kind == "ln":
            x = x[:1].expand(W4.M_MAX, K)
        x, bias = x.double(), bias.double()
        absdot = x.abs() @ weff.abs().t()
        ref = x @ weff.t() + bias
        bnd = GC.bound(ref, absdot, bias, K, dtype, x_rounded=kind == "attn").cuda()
        ref_d, gelu_ref = ref.cuda(), O.gelu(ref.float())
        for M in W4.MS:
            for N in W4.NS:
                rc, out = W4.plan(kind, dtype, M, N, K)
                if rc != 0:
                    continue
                form = GC.form_name(out)
                where = f"M={M} N={N} K={K} [{form}]"
                got = prod(M, N)
                ratio = float(((got.double() - ref_d[:M, :N]).abs() / bnd[:M, :N]).max())
                worst[form] = max(worst.get(form, 0.0), ratio)
                if not ratio <= 1.0:
                    fails.append(f"{where}: err / bound = {ratio:.3f}")
                if kind != "attn":
                    e = rel(prod(M, N, gelu=True), gelu_ref[:M, :N])
                    if not e < TOL[dtype]:
                        fails.append(f"{where}: GeLU output rel-L2 {e:.2e}")
    for form, r in sorted(worst.items()):
        print(f"RATIO mxfp4 {form} {kind} {GC.DT_NAME[dtype]}: worst err / bound = {r:.4f}")
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("dtype", W4.DTYPES, ids=GC.DT_NAME.get)
@pytest.mark.parametrize("M", [1, 2, 4, 8])
@pytest.mark.parametrize("H", [16, 40, 24])                        # K = 1024, 2560 and a guarded K (1536)
def test_combine_prologue_form_equals_the_two_launch_form(ops, dtype, M, H):
    cap, pos, N = 256, 100, 136
    g = torch.Generator().manual_seed(cap + pos + N + H + M)
    hp = H * 64
    cache, qkv = rnd((M, cap, 2 * hp), dtype, g), rnd((M, 1, 3 * hp), dtype, g)
    w, bias = rnd((N, hp), dtype, g, 0.05), rnd((N,), dtype, g)
    qs = ops.quantize_rows_mxfp4(w.cuda())
    pos_d = torch.tensor([pos], dtype=torch.int64, device="cuda")
    c1, c2 = cache.clone().cuda(), cache.clone().cuda()
    att = ops.attention_decode(qkv.cuda(), c1, pos_d, H)           # the existing combine launch
    slot_ref = ops.new_absmax_slot(att.device)
    ref2 = ops.gemm_w4(att.view(M, hp), qs, bias=bias.cuda(), absmax=slot_ref)
    parts = ops.attention_decode(qkv.cuda(), c2, pos_d, H, combine=False)
    slot = ops.new_absmax_slot(att.device)
    out = ops.gemv_attn_w4(parts, M, H, cap, qs, dtype, bias=bias.cuda(), absmax=slot)
    assert out.shape == (M, N) and out.dtype == dtype and torch.equal(out, ref2)
    assert slot.item() == slot_ref.item()
    ref = att.view(M, hp).double().cpu() @ W4.dequantize(*qs).t() + bias.double()
    assert rel(out, ref) < TOL[dtype]
    assert torch.equal(out, ops.gemv_attn_w4(parts, M, H, cap, qs, dtype, bias=bias.cuda()))


@pytest.mark.parametrize("dtype", W4.DTYPES, ids=GC.DT_NAME.get)
@pytest.mark.parametrize("stream32", [False, True])
@pytest.mark.parametrize("M,K,N,post,gelu", [(1, 512, 8, False, False), (1, 1024, 40, True, True), (1, 2560, 136, True, False),
                                              (2, 1024, 136, False, True), (2, 4096, 40, True, True), (3, 2560, 40, True, True),
                                              (4, 1536, 136, True, False), (5, 2560, 136, False, True), (8, 1024, 40, True, False),
                                              (1, 4096, 136, False, True)])
def test_layernorm_prologue_form_against_its_composition(ops, dtype, stream32, M, K, N, post, gelu):
    """cogv_gemv_ln_w4 == the existing Sandwich-LN launches followed by the plain 4-bit product: the cases and bars of
    tests/test_w8_gemv_gpu.py's test of the same name."""
    g = torch.Generator().manual_seed(M * 100 + K + N)
    z = rnd((M, K), torch.float32 if (stream32 and not post) else dtype, g, 3.0)
    res = rnd((M, K), torch.float32 if stream32 else dtype, g)
    w, bias = rnd((N, K), dtype, g, 0.05), rnd((N,), dtype, g)
    gp, bp = (1.0 + 0.1 * torch.randn(K, generator=g)).to(dtype).cuda(), (0.1 * torch.randn(K, generator=g)).to(dtype).cuda()
    gn, bn = (1.0 + 0.1 * torch.randn(K, generator=g)).to(dtype).cuda(), (0.1 * torch.randn(K, generator=g)).to(dtype).cuda()
    eps = 1e-5
    qs = ops.quantize_rows_mxfp4(w.cuda())
    zd, resd, bd = z.cuda(), res.cuda(), bias.cuda()
    zmax = ops.absmax(zd)
    if post:
        slot_t = ops.new_absmax_slot(zd.device)
        t_ref, _, _ = ops.sandwich_ln_fwd(zd, gp, bp, eps, zmax, residual=resd, absmax_out=slot_t, save_stats=False)
    else:
        t_ref, slot_t = zd, zmax
    x_ref, _, _ = ops.sandwich_ln_fwd(t_ref, gn, bn, eps, slot_t, save_stats=False)
    slot_ref = ops.new_absmax_slot(zd.device)
    out_ref = ops.gemm_w4(x_ref, qs, bias=bd, gelu=gelu, absmax=slot_ref)
    slot = ops.new_absmax_slot(zd.device)
    out, t = ops.gemv_ln_w4(zd, qs, bd, gn, bn, eps, z_absmax=zmax, post=(gp, bp) if post else None,
                            residual=resd if post else None, want_t=post, gelu=gelu, absmax=slot)
    if post:
        if stream32:
            assert t.dtype == torch.float32 and rel(t, t_ref) < 1e-6
        else:
            assert torch.equal(t, t_ref), "the residual stream written by workgroup 0 must equal the LayerNorm kernel's"
        out2, t2 = ops.gemv_ln_w4(zd, qs, bd, gn, bn, eps, z_absmax=None, post=(gp, bp), residual=resd, want_t=True, gelu=gelu)
        assert torch.equal(out2, out) and torch.equal(t2, t)
        out3, t3 = ops.gemv_ln_w4(zd, qs, bd, gn, bn, eps, z_absmax=zmax, post=(gp, bp), residual=resd, want_t=False, gelu=gelu)
        assert t3 is None and torch.equal(out3, out)
    else:
        assert t is None
    e = rel(out, out_ref)
    print(f"[{dtype}] stream32={stream32} M={M} K={K} N={N} post={post} gelu={gelu}: rel-L2 vs composition {e:.2e}")
    assert out.dtype == dtype and e < TOL_LN[dtype]
    assert abs(slot.item() - slot_ref.item()) <= 2e-2 * max(1.0, slot_ref.item())
    ref = x_ref.double().cpu() @ W4.dequantize(*qs).t() + bias.double()
    if gelu:
        ref = O.gelu(ref.to(dtype).float())
    assert rel(out, ref) < TOL[dtype]


@pytest.mark.parametrize("dtype", W4.DTYPES, ids=GC.DT_NAME.get)
@pytest.mark.parametrize("M,K", [(1, 1024), (1, 1536), (3, 2560), (8, 4096)])
def test_strided_operands_inside_sentinel_buffers(ops, dtype, M, K):
    """x rows lda = K + 8 apart, codes ldq = K / 2 + 16, block scales lds = K / 32 + 5, output rows ldc = N + 8: the exact-integer
    product still equals fp64 to the bit, and no byte around the output moves."""
    import ctypes as C
    from cogview_amd import _lib as L
    N = 40
    x, (q, s), w, bias, dot = W4.exact_operands(K, dtype)
    ref = (dot + bias)[:M, :N].to(dtype)
    dev = "cuda"
    xb = torch.full((M, K + 8), 3.0, dtype=dtype, device=dev)
    xb[:, :K] = x[:M].to(dtype)
    qb = torch.full((N + 1, K // 2 + 16), 0x77, dtype=torch.uint8, device=dev)          # 0x77: two codes of 6.0 where nothing may read
    qb[:N, :K // 2] = q[:N]
    sb = torch.full((N + 1, K // 32 + 5), 254, dtype=torch.uint8, device=dev)
    sb[:N, :K // 32] = s[:N]
    cb = torch.full((M + 2, N + 8), -7.0, dtype=dtype, device=dev)
    out = cb[1:M + 1, :N]
    bias_d = bias[:N].to(dtype).to(dev)
    d = ops._skinny_desc(out, K, bias_d, False, None)
    d.A, d.lda, d.ldc = xb.data_ptr(), xb.stride(0), cb.stride(0)
    wq = L.W4Weight()
    wq.q, wq.ldq, wq.scale, wq.lds = qb.data_ptr(), qb.stride(0), sb.data_ptr(), sb.stride(0)
    assert d.ldc == N + 8 and d.M == M and d.N == N
    L.check(L.lib().cogv_gemm_w4(C.byref(d), C.byref(wq), None), "cogv_gemm_w4")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref)
    assert bool((cb[0] == -7.0).all() and (cb[-1] == -7.0).all() and (cb[:, N:] == -7.0).all())
    # the same through ops on strided views
    got = ops.gemm_w4(xb[:, :K], (qb[:N, :K // 2], sb[:N, :K // 32]), bias=bias_d)
    assert torch.equal(got.cpu(), ref)


def test_unsupported_shapes_raise(ops):
    from cogview_amd._lib import CogviewHipError

    def call(M, N, K):
        q = torch.zeros((N, K // 2), dtype=torch.uint8, device="cuda")
        s = torch.full((N, K // 32), 127, dtype=torch.uint8, device="cuda")
        return ops.gemm_w4(torch.zeros((M, K), dtype=torch.float16, device="cuda"), (q, s))

    assert call(8, 8, 512).shape == (8, 8)
    for M, N, K in ((1, 8, 768), (1, 12, 512), (9, 8, 512), (2, 8, 5632), (8, 8, 5120), (1, 8, 10752)):
        with pytest.raises(CogviewHipError, match="unsupported"):
            call(M, N, K)
