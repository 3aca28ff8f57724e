"""GPU: the skinny-M products on an 8-bit (E4M3, one scale per row) weight operand -- cogv_gemm_w8, cogv_gemv_ln_w8,
cogv_gemv_attn_w8 through ops.  The oracle multiplies x with q.float() * scale in fp64: the quantized weights are exact on
both sides, so the kernels are held to the bars tests/test_kernels_gpu.py sets for the 16-bit skinny-M kernels
(relative L2: fp16 3e-3, bf16 2e-2; LayerNorm-prologue form against its composition: 2e-3 / 1.5e-2)."""
import pytest
import torch

from oracle import cogview_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
TOL = {torch.float16: 3e-3, torch.bfloat16: 2e-2}                 # tests/test_kernels_gpu.py
TOL_LN = {torch.float16: 2e-3, torch.bfloat16: 1.5e-2}            # test_gemv_with_layernorm_prologue, against the composition
E4M3 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops as _ops
    return _ops


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def rnd(shape, dtype, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(dtype)


def dequant(qs):
    """the weights the 8-bit kernels see, in fp64"""
    q, scale = qs
    return q.cpu().view(E4M3).double() * scale.cpu().double()[:, None]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [512, 1024, 1536, 2560, 4096, 10240])
@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 8])
def test_plain_product_against_the_fp64_oracle(ops, dtype, M, K):
    for N in (8, 40, 136):                                         # 40: ragged against every columns-per-workgroup choice
        g = torch.Generator().manual_seed(M * 31 + N + K)
        a, w, bias = rnd((M, K), dtype, g), rnd((N, K), dtype, g, 0.1), rnd((N,), dtype, g)
        qs = ops.quantize_rows_e4m3(w.cuda())
        wq = dequant(qs)
        ref = a.double() @ wq.t()
        ad, bd = a.cuda(), bias.cuda()
        e0 = rel(ops.gemm_w8(ad, qs), ref)
        slot = torch.zeros(1, dtype=torch.float32, device="cuda")
        out = ops.gemm_w8(ad, qs, bias=bd, absmax=slot)
        e1 = rel(out, ref + bias.double())
        act = ops.gemm_w8(ad, qs, bias=bd, gelu=True)
        e2 = rel(act, O.gelu((ref + bias.double()).float()))
        print(f"[{dtype}] M={M} K={K} N={N}: rel-L2 plain {e0:.2e} bias {e1:.2e} gelu {e2:.2e}")
        assert out.dtype == dtype and out.shape == (M, N)
        assert e0 < TOL[dtype] and e1 < TOL[dtype] and e2 < TOL[dtype], (N, e0, e1, e2)
        assert abs(slot.item() - out.float().abs().max().item()) <= 1e-6 * max(1.0, slot.item())
        assert torch.equal(out, ops.gemm_w8(ad, qs, bias=bd))


@pytest.mark.parametrize("M", [1, 2])
def test_decode_table(ops, M):
    """Every non-NaN E4M3 byte through a K = 512 product against a one-hot x: the result is torch's float8_e4m3fn -> float
    table, exactly (scale 1, fp16 output: every E4M3 value is an fp16 value) -- at every element position of a lane's load."""
    table = torch.arange(256, dtype=torch.uint8)
    finite = (table & 0x7f) != 0x7f
    assert int(finite.sum()) == 254
    want = torch.where(finite, table.view(E4M3).float(), torch.zeros(256))
    scale = torch.ones(256, dtype=torch.float32, device="cuda")
    for k0 in list(range(16)) + [8 * 37 + 3, 255, 256, 511]:
        q = torch.zeros((256, 512), dtype=torch.uint8)
        q[:, k0] = torch.where(finite, table, torch.zeros(256, dtype=torch.uint8))
        q[:, (k0 + 9) % 512] = 0x38                                # 1.0 in a column x does not select
        x = torch.zeros((M, 512), dtype=torch.float16)
        x[:, k0] = 1.0
        out = ops.gemm_w8(x.cuda(), (q.cuda(), scale)).cpu().float()
        for m in range(M):
            assert torch.equal(out[m], want), (k0, m, (out[m] != want).nonzero().flatten().tolist()[:8])
        # (value equality: byte 0x80 is -0.0, and a sum that starts at +0.0 ends at +0.0 -- IEEE: +0 + (-0) = +0 -- as in the
        #  16-bit kernels; the sign of a zero weight cannot show in a dot product)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 2, 4, 8])
@pytest.mark.parametrize("H", [16, 40, 24])                        # K = 1024, 2560 and a guarded K (1536)
def test_combine_prologue_form_equals_the_two_launch_form(ops, dtype, M, H):
    cap, pos, N = 256, 100, 136
    g = torch.Generator().manual_seed(cap + pos + N + H + M)
    hp = H * 64
    cache, qkv = rnd((M, cap, 2 * hp), dtype, g), rnd((M, 1, 3 * hp), dtype, g)
    w, bias = rnd((N, hp), dtype, g, 0.05), rnd((N,), dtype, g)
    qs = ops.quantize_rows_e4m3(w.cuda())
    pos_d = torch.tensor([pos], dtype=torch.int64, device="cuda")
    c1, c2 = cache.clone().cuda(), cache.clone().cuda()
    att = ops.attention_decode(qkv.cuda(), c1, pos_d, H)           # the existing combine launch
    slot_ref = ops.new_absmax_slot(att.device)
    ref2 = ops.gemm_w8(att.view(M, hp), qs, bias=bias.cuda(), absmax=slot_ref)
    parts = ops.attention_decode(qkv.cuda(), c2, pos_d, H, combine=False)
    slot = ops.new_absmax_slot(att.device)
    out = ops.gemv_attn_w8(parts, M, H, cap, qs, dtype, bias=bias.cuda(), absmax=slot)
    assert out.shape == (M, N) and out.dtype == dtype and torch.equal(out, ref2)
    assert slot.item() == slot_ref.item()
    ref = att.view(M, hp).double().cpu() @ dequant(qs).t() + bias.double()
    assert rel(out, ref) < TOL[dtype]
    assert torch.equal(out, ops.gemv_attn_w8(parts, M, H, cap, qs, dtype, bias=bias.cuda()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stream32", [False, True])
@pytest.mark.parametrize("M,K,N,post,gelu", [(1, 512, 8, False, False), (1, 1024, 40, True, True), (1, 2560, 136, True, False),
                                              (2, 1024, 136, False, True), (2, 4096, 40, True, True), (3, 2560, 40, True, True),
                                              (4, 1536, 136, True, False), (5, 2560, 136, False, True), (8, 1024, 40, True, False),
                                              (1, 4096, 136, False, True)])
def test_layernorm_prologue_form_against_its_composition(ops, dtype, stream32, M, K, N, post, gelu):
    """cogv_gemv_ln_w8 == the existing Sandwich-LN launches followed by the plain 8-bit product (the criterion of
    test_gemv_with_layernorm_prologue): post-LN + residual and plain input, t written once, all-16-bit and fp32 stream."""
    g = torch.Generator().manual_seed(M * 100 + K + N)
    z = rnd((M, K), torch.float32 if (stream32 and not post) else dtype, g, 3.0)
    res = rnd((M, K), torch.float32 if stream32 else dtype, g)
    w, bias = rnd((N, K), dtype, g, 0.05), rnd((N,), dtype, g)
    gp, bp = (1.0 + 0.1 * torch.randn(K, generator=g)).to(dtype).cuda(), (0.1 * torch.randn(K, generator=g)).to(dtype).cuda()
    gn, bn = (1.0 + 0.1 * torch.randn(K, generator=g)).to(dtype).cuda(), (0.1 * torch.randn(K, generator=g)).to(dtype).cuda()
    eps = 1e-5
    qs = ops.quantize_rows_e4m3(w.cuda())
    zd, resd, bd = z.cuda(), res.cuda(), bias.cuda()
    zmax = ops.absmax(zd)
    if post:
        slot_t = ops.new_absmax_slot(zd.device)
        t_ref, _, _ = ops.sandwich_ln_fwd(zd, gp, bp, eps, zmax, residual=resd, absmax_out=slot_t, save_stats=False)
    else:
        t_ref, slot_t = zd, zmax
    x_ref, _, _ = ops.sandwich_ln_fwd(t_ref, gn, bn, eps, slot_t, save_stats=False)
    slot_ref = ops.new_absmax_slot(zd.device)
    out_ref = ops.gemm_w8(x_ref, qs, bias=bd, gelu=gelu, absmax=slot_ref)
    slot = ops.new_absmax_slot(zd.device)
    out, t = ops.gemv_ln_w8(zd, qs, bd, gn, bn, eps, z_absmax=zmax, post=(gp, bp) if post else None,
                            residual=resd if post else None, want_t=post, gelu=gelu, absmax=slot)
    if post:
        if stream32:
            assert t.dtype == torch.float32 and rel(t, t_ref) < 1e-6          # test_gemv_layernorm_prologue_on_the_fp32_stream
        else:
            assert torch.equal(t, t_ref), "the residual stream written by workgroup 0 must equal the LayerNorm kernel's"
        out2, t2 = ops.gemv_ln_w8(zd, qs, bd, gn, bn, eps, z_absmax=None, post=(gp, bp), residual=resd, want_t=True, gelu=gelu)
        assert torch.equal(out2, out) and torch.equal(t2, t)
        out3, t3 = ops.gemv_ln_w8(zd, qs, bd, gn, bn, eps, z_absmax=zmax, post=(gp, bp), residual=resd, want_t=False, gelu=gelu)
        assert t3 is None and torch.equal(out3, out)
    else:
        assert t is None
    e = rel(out, out_ref)
    print(f"[{dtype}] stream32={stream32} M={M} K={K} N={N} post={post} gelu={gelu}: rel-L2 vs composition {e:.2e}")
    assert out.dtype == dtype and e < TOL_LN[dtype]
    assert abs(slot.item() - slot_ref.item()) <= 2e-2 * max(1.0, slot_ref.item())
    # and the fp64 product of the composition's own x_in with the quantized weights
    ref = x_ref.double().cpu() @ dequant(qs).t() + bias.double()
    if gelu:
        ref = O.gelu(ref.to(dtype).float())
    assert rel(out, ref) < TOL[dtype]


def test_unsupported_shapes_raise(ops):
    from cogview_amd._lib import CogviewHipError

    def call(M, N, K):
        q = torch.zeros((N, K), dtype=torch.uint8, device="cuda")
        s = torch.ones(N, dtype=torch.float32, device="cuda")
        return ops.gemm_w8(torch.zeros((M, K), dtype=torch.float16, device="cuda"), (q, s))

    assert call(8, 8, 512).shape == (8, 8)
    for M, N, K in ((1, 8, 768), (1, 12, 512), (9, 8, 512)):       # K % 512, N % 8, M > 8
        with pytest.raises(CogviewHipError, match="unsupported"):
            call(M, N, K)
