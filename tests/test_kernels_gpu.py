"""GPU parity: every HIP kernel (through the C ABI) against the CPU oracle on seeded inputs.

Tolerances (relative L2 error ||hip - oracle|| / ||oracle||, oracle in fp32 on the inputs rounded to the
storage type): fp16 3e-3, bf16 2e-2 for single kernels whose output is rounded once to 16 bits
(bf16 has 8 significant bits: 2^-9 = 2e-3 per element before any accumulation effects).
The Sandwich-LN kernels are judged element by element, every form and loop path, by tests/test_layernorm_cells_gpu.py.
"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import cogview_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
TOL = {torch.float16: 3e-3, torch.bfloat16: 2e-2}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops as _ops
    return _ops


def dev(t):
    return t.cuda()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def rnd(shape, dtype, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(dtype)


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (510, 768, 256), (300, 136, 72), (1088, 1024, 1024), (64, 2560, 2560),
                                   (700, 520, 192), (2000, 264, 64)])
def test_gemm_nt_bias(ops, dtype, M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N)
    a, b, bias = rnd((M, K), dtype, g), rnd((N, K), dtype, g, 0.1), rnd((N,), dtype, g)
    ref = O.linear(a.float(), b.float(), bias.float())
    out = ops.gemm(dev(a), dev(b), bias=dev(bias))
    assert rel(out, ref) < TOL[dtype]
    out1 = ops.gemm(dev(a), dev(b), bias=dev(bias), splitk=1)
    assert rel(out1, ref) < TOL[dtype]
    if M >= 256 and N >= 256 and K % 64 == 0:      # the explicit kernel generations (default dispatch picks 4)
        for variant in (9, 10):
            assert rel(ops.gemm(dev(a), dev(b), bias=dev(bias), variant=variant), ref) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_asymmetric_identity(ops, dtype):
    """A = I with an asymmetric B catches transposed C writes / operand swaps."""
    n = 256
    a = torch.eye(n).to(dtype)
    b = (torch.arange(n).view(n, 1) * 0.01 + torch.arange(n).view(1, n) * 0.5).to(dtype)   # b[j][k]
    out = ops.gemm(dev(a), dev(b))          # C[m][j] = sum_k I[m][k] b[j][k] = b[j][m]
    assert torch.equal(out.cpu(), b.t().contiguous())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(510, 256, 768), (1088, 1024, 3072), (136, 72, 304), (700, 520, 192)])
def test_gemm_dgrad_nn(ops, dtype, M, N, K):
    """dX[M,N] = dY[M,K] W[K,N]  (trans_b: B stored [K][N])."""
    g = torch.Generator().manual_seed(K)
    dy, w = rnd((M, K), dtype, g), rnd((K, N), dtype, g, 0.1)
    ref = dy.float() @ w.float()
    assert rel(ops.gemm(dev(dy), dev(w), trans_b=True), ref) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K,splitk", [(768, 256, 510, 1), (1024, 1024, 4352, None), (72, 136, 300, 3), (3072, 1024, 2176, 4),
                                          (520, 264, 1088, 2), (2560, 2560, 8704, None)])
def test_gemm_wgrad_tn(ops, dtype, M, N, K, splitk):
    """dW[M,N] = dY[K,M]^T X[K,N]  (both operands stored contraction-major)."""
    g = torch.Generator().manual_seed(K + 1)
    dy, x = rnd((K, M), dtype, g), rnd((K, N), dtype, g)
    ref = dy.float().t() @ x.float()
    out = ops.gemm(dev(dy), dev(x), trans_a=True, trans_b=True, splitk=splitk)
    assert rel(out, ref) < TOL[dtype]
    # accumulate into an existing gradient
    prev = rnd((M, N), dtype, g, 5.0)
    acc = dev(prev.clone())
    ops.gemm(dev(dy), dev(x), trans_a=True, trans_b=True, out=acc, accumulate=True, splitk=splitk)
    assert rel(acc, ref + prev.float()) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(512, 768, 320), (264, 136, 200)])
def test_gemm_a_transposed_only(ops, dtype, M, N, K):
    """C[M,N] = A[K,M]^T B[N,K]^T: the fourth operand layout of the C ABI (trans_a without trans_b; no caller on the
    training path, but every layout of every kernel generation is a separate instantiation)."""
    g = torch.Generator().manual_seed(K + 3)
    a, b = rnd((K, M), dtype, g), rnd((N, K), dtype, g, 0.1)
    ref = a.float().t() @ b.float().t()
    assert rel(ops.gemm(dev(a), dev(b), trans_a=True), ref) < TOL[dtype]
    assert rel(ops.gemm(dev(a), dev(b), trans_a=True, variant=9), ref) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [1088, 4352])
def test_gemm_grouped_wgrads(ops, dtype, K):
    """The four weight gradients of a layer in one persistent launch (cogv_gemm_grouped) == four separate GEMMs,
    bit for bit when no split is chosen, and within tolerance of the fp32 reference either way."""
    g = torch.Generator().manual_seed(K)
    shapes = [(768, 256), (256, 256), (1024, 256), (256, 1024)]          # (out features, in features)
    probs, refs, singles = [], [], []
    for M, N in shapes:
        dy, x, prev = rnd((K, M), dtype, g), rnd((K, N), dtype, g), rnd((M, N), dtype, g, 3.0)
        refs.append(dy.float().t() @ x.float() + prev.float())
        probs.append((dev(dy), dev(x), dev(prev.clone())))
        one = dev(prev.clone())
        ops.gemm(dev(dy), dev(x), trans_a=True, trans_b=True, out=one, accumulate=True, splitk=1, variant=9)
        singles.append(one)
    ops.gemm_grouped(probs, trans_a=True, trans_b=True, accumulate=True)
    for (_, _, out), ref, one in zip(probs, refs, singles):
        assert rel(out, ref) < TOL[dtype]
        assert rel(out, one.float()) < 2e-3
    # shapes the grouped kernel does not take fall back to one launch per problem
    dy, x = rnd((300, 72), dtype, g), rnd((300, 136), dtype, g)
    out = torch.zeros(72, 136, dtype=dtype).cuda()
    ops.gemm_grouped([(dev(dy), dev(x), out)], trans_a=True, trans_b=True, accumulate=True)
    assert rel(out, dy.float().t() @ x.float()) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(1088, 1024, 256), (700, 512, 192), (300, 136, 72)])
def test_gemm_fused_colsum(ops, dtype, M, N, K):
    """COGV_EPI_COLSUM: the bias gradient (column sums of the rounded dgrad output) from the GEMM epilogue equals
    the separate column-sum pass over the stored output; shapes the fused path does not take fall back to it."""
    g = torch.Generator().manual_seed(N + K)
    dy, w, u = rnd((M, K), dtype, g), rnd((K, N), dtype, g, 0.1), rnd((M, N), dtype, g)
    prev = rnd((N,), dtype, g)
    fused = dev(prev.clone())
    out = ops.gemm(dev(dy), dev(w), trans_b=True, dgelu_aux=dev(u), colsum_out=fused)
    ref_out = ops.gemm(dev(dy), dev(w), trans_b=True, dgelu_aux=dev(u))
    assert torch.equal(out, ref_out)
    sep = dev(prev.clone())
    ops.colsum(ref_out, out=sep, accumulate=True)
    expect = ref_out.float().sum(0).cpu() + prev.float()
    assert rel(fused, expect) < TOL[dtype]
    assert rel(fused, sep.float()) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_gelu_dgelu_epilogues(ops, dtype):
    g = torch.Generator().manual_seed(3)
    M, N, K = 320, 512, 128
    a, w, bias = rnd((M, K), dtype, g), rnd((N, K), dtype, g, 0.2), rnd((N,), dtype, g)
    u_ref = O.linear(a.float(), w.float(), bias.float())
    aux = torch.empty((M, N), dtype=dtype, device="cuda")
    out = ops.gemm(dev(a), dev(w), bias=dev(bias), gelu=True, gelu_aux=aux)
    assert rel(aux, u_ref) < TOL[dtype]
    assert rel(out, O.gelu(aux.float().cpu())) < TOL[dtype]          # activation of the stored pre-activation
    # dgelu epilogue: out = (dy @ w2) * gelu'(u)
    dy, w2 = rnd((M, K), dtype, g), rnd((K, N), dtype, g, 0.2)
    u = aux.float().cpu().requires_grad_(True)
    O.gelu(u).backward(torch.ones_like(u))
    ref = (dy.float() @ w2.float()) * u.grad
    out2 = ops.gemm(dev(dy), dev(w2), trans_b=True, dgelu_aux=aux)
    assert rel(out2, ref) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(320, 512, 128), (1088, 2560, 256), (5, 512, 1024)])
def test_gelu_epilogue_forms_differ_by_at_most_one_rounding_of_the_preactivation(ops, dtype, M, N, K):
    """The three GeLU epilogue forms and their rounding points ("Rounding points of GeLU"): the training form
    (stored derivative, COGV_EPI_GELU_DAUX) and the inference form (nothing stored) evaluate the activation on the fp32
    pre-activation -- identical bits; the stored-pre-activation form (and the reference: fp16 Linear output, then gelu,
    mpu/sparse_transformer.py:172-179, :239-244) evaluates it on the pre-activation ROUNDED to the storage type.  The two families
    therefore differ by at most the effect of that one rounding: |d gelu| <= max|gelu'| (1.13) * half an ulp of the pre-activation,
    plus the output's own rounding -- bounded here element by element."""
    g = torch.Generator().manual_seed(M + N + K)
    a, w, bias = rnd((M, K), dtype, g), rnd((N, K), dtype, g, 0.2), rnd((N,), dtype, g)
    daux = torch.empty((M, N), dtype=dtype, device="cuda")
    aux = torch.empty((M, N), dtype=dtype, device="cuda")
    train = ops.gemm(dev(a), dev(w), bias=dev(bias), gelu=True, gelu_daux=daux)
    infer = ops.gemm(dev(a), dev(w), bias=dev(bias), gelu=True)
    stored = ops.gemm(dev(a), dev(w), bias=dev(bias), gelu=True, gelu_aux=aux)
    assert torch.equal(train, infer)
    eps = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8            # half an ulp, relative
    u = aux.float().abs()
    bound = 1.13 * eps * u + eps * stored.float().abs() * 2 + 1e-7          # pre-activation rounding through gelu' + two output roundings
    diff = (train.float() - stored.float()).abs()
    assert bool((diff <= bound).all()), float((diff - bound).max())
    assert rel(train, stored) < (6e-4 if dtype == torch.float16 else 5e-3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(320, 512, 128), (1088, 1024, 256), (300, 136, 72)])
def test_gemm_stored_gelu_derivative_epilogues(ops, dtype, M, N, K):
    """COGV_EPI_GELU_DAUX / COGV_EPI_MULAUX (the fused layer's pair): the forward epilogue stores gelu'(pre-activation)
    and returns the activation of the fp32 pre-activation (round 3: no rounding of the pre-activation in between -- the plain
    epilogue, which STORES the pre-activation, evaluates GeLU on the stored, rounded value); the backward epilogue multiplies by the
    stored derivative (and still produces the fused bias-gradient column sums) -- against the oracle's autograd of
    gelu (mpu/sparse_transformer.py:172-179)."""
    g = torch.Generator().manual_seed(M + N)
    a, w, bias = rnd((M, K), dtype, g), rnd((N, K), dtype, g, 0.2), rnd((N,), dtype, g)
    u_aux = torch.empty((M, N), dtype=dtype, device="cuda")
    plain = ops.gemm(dev(a), dev(w), bias=dev(bias), gelu=True, gelu_aux=u_aux)
    d_aux = torch.empty((M, N), dtype=dtype, device="cuda")
    out = ops.gemm(dev(a), dev(w), bias=dev(bias), gelu=True, gelu_daux=d_aux)
    pre = O.linear(a.float(), w.float(), bias.float())
    assert rel(out, O.gelu(pre)) < TOL[dtype] and rel(out, plain.float().cpu()) < TOL[dtype]
    assert rel(out, O.gelu(pre)) <= rel(plain, O.gelu(pre)) * 1.05         # at least as close to the fp32 definition
    none = ops.gemm(dev(a), dev(w), bias=dev(bias), gelu=True)             # nothing stored (inference): same fp32 evaluation
    assert torch.equal(none, out)
    u = u_aux.float().cpu().requires_grad_(True)
    O.gelu(u).backward(torch.ones_like(u))
    assert rel(d_aux, u.grad) < TOL[dtype]
    dy, w2 = rnd((M, K), dtype, g), rnd((K, N), dtype, g, 0.2)
    ref = (dy.float() @ w2.float()) * u.grad
    cs = torch.zeros(N, dtype=dtype, device="cuda")
    out2 = ops.gemm(dev(dy), dev(w2), trans_b=True, mul_aux=d_aux, colsum_out=cs, colsum_accumulate=False)
    assert rel(out2, ref) < 1.5 * TOL[dtype]              # two 16-bit roundings (stored derivative, output)
    assert rel(cs, out2.float().sum(0)) < TOL[dtype]
    old = ops.gemm(dev(dy), dev(w2), trans_b=True, dgelu_aux=u_aux)
    assert rel(out2, old.float().cpu()) < 1.5 * TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("N,K", [(768, 512), (2560, 2560), (136, 1024), (24, 2560), (40, 4096), (264, 1536), (2560, 10240), (64, 10752)])
def test_gemm_skinny_m_decode_shapes(ops, dtype, M, N, K):
    """M <= 8 (one row per beam in a decode step) runs the HBM-streaming matrix-vector kernel; it must agree with the
    tile kernels' results (explicit kernel_variant) and the oracle through the same fused epilogues."""
    g = torch.Generator().manual_seed(M * 31 + N + K)
    a, w, bias = rnd((M, K), dtype, g), rnd((N, K), dtype, g, 0.1), rnd((N,), dtype, g)
    ref = O.linear(a.float(), w.float(), bias.float())
    slot = torch.zeros(1, dtype=torch.float32, device="cuda")
    out = ops.gemm(dev(a), dev(w), bias=dev(bias), absmax=slot)
    assert rel(out, ref) < TOL[dtype]
    assert abs(slot.item() - out.float().abs().max().item()) <= 1e-6 * max(1.0, slot.item())
    tiles = ops.gemm(dev(a), dev(w), bias=dev(bias), variant=1, splitk=1)          # generation-1 tile kernel
    assert rel(out, tiles.float().cpu()) < TOL[dtype]
    aux = torch.empty((M, N), dtype=dtype, device="cuda")
    act = ops.gemm(dev(a), dev(w), bias=dev(bias), gelu=True, gelu_aux=aux)
    assert rel(aux, ref) < TOL[dtype] and rel(act, O.gelu(aux.float().cpu())) < TOL[dtype]
    assert rel(ops.gemm(dev(a), dev(w)), a.float() @ w.float().t()) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_dropout_absmax(ops, dtype):
    g = torch.Generator().manual_seed(4)
    M, N, K = 200, 384, 64
    a, w = rnd((M, K), dtype, g), rnd((N, K), dtype, g)
    ref = a.float() @ w.float().t()
    mask = torch.from_numpy(O.dropout_keep_mask(M * N, 0.1, 99, 5)).view(M, N)
    slot = ops.new_absmax_slot(torch.device("cuda"))
    out = ops.gemm(dev(a), dev(w), dropout=(0.1, 99, 5), absmax=slot)
    assert torch.equal((out.cpu() == 0), (mask == 0) | (out.cpu() == 0))
    assert rel(out, ref * mask) < TOL[dtype]
    assert abs(slot.item() - out.float().abs().max().item()) == 0.0


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,h", [(60, 128), (1088, 1024), (257, 2560), (33, 256), (17, 4096)])
def test_sandwich_ln_fwd_bwd(ops, dtype, rows, h):
    g = torch.Generator().manual_seed(h + rows)
    x = rnd((rows, h), dtype, g, 3.0)
    w = (torch.rand(h, generator=g) + 0.5).to(dtype)
    b = rnd((h,), dtype, g, 0.1)
    dy = rnd((rows, h), dtype, g)
    xr, wr, br = x.float().requires_grad_(True), w.float().requires_grad_(True), b.float().requires_grad_(True)
    yr = O.sandwich_layernorm(xr, wr, br, 1e-5)
    yr.backward(dy.float())
    xd = dev(x)
    amax = ops.absmax(xd)
    assert amax.item() == x.float().abs().max().item()
    y, mean, rstd = ops.sandwich_ln_fwd(xd, dev(w), dev(b), 1e-5, amax)
    assert rel(y, yr) < TOL[dtype]
    dg = torch.zeros(h, dtype=dtype, device="cuda")
    db = torch.zeros(h, dtype=dtype, device="cuda")
    dx = ops.sandwich_ln_bwd(dev(dy), xd, dev(w), mean, rstd, dgamma=dg, dbeta=db)
    assert rel(dx, xr.grad) < TOL[dtype] * 2
    assert rel(dg, wr.grad) < TOL[dtype] * 2
    assert rel(db, br.grad) < TOL[dtype] * 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_sandwich_ln_fused_residual_dropout_colsum(ops, dtype):
    g = torch.Generator().manual_seed(11)
    rows, h = 300, 512
    x, res = rnd((rows, h), dtype, g, 2.0), rnd((rows, h), dtype, g)
    w, b = (torch.rand(h, generator=g) + 0.5).to(dtype), rnd((h,), dtype, g, 0.1)
    xd = dev(x)
    amax = ops.absmax(xd)
    slot = ops.new_absmax_slot(xd.device)
    y, mean, rstd = ops.sandwich_ln_fwd(xd, dev(w), dev(b), 1e-5, amax, residual=dev(res), absmax_out=slot)
    ln = O.sandwich_layernorm(x.float(), w.float(), b.float()).to(dtype).float()
    assert rel(y, res.float() + ln) < TOL[dtype]
    assert slot.item() == y.float().abs().max().item()
    # backward with dropout mask replay, residual-gradient add and column sums
    dy, add_in = rnd((rows, h), dtype, g), rnd((rows, h), dtype, g)
    xr = x.float().requires_grad_(True)
    O.sandwich_layernorm(xr, w.float(), b.float()).backward(dy.float())
    mask = torch.from_numpy(O.dropout_keep_mask(rows * h, 0.1, 7, 3)).view(rows, h)
    cs = torch.zeros(h, dtype=dtype, device="cuda")
    dx = ops.sandwich_ln_bwd(dev(dy), xd, dev(w), mean, rstd, add_in=dev(add_in), dropout=(0.1, 7, 3), colsum=cs)
    ref = xr.grad * mask + add_in.float()
    assert rel(dx, ref) < TOL[dtype] * 2
    assert rel(cs, dx.float().cpu().sum(0)) < TOL[dtype] * 2


# ------------------------------------------------------------------------------------------------ attention
def _attn_ref(q, k, v, sep, drop=None, dout=None):
    """q,k,v [b,s,H,64] -> oracle on [b,H,s,64]."""
    qr, kr, vr = [t.float().permute(0, 2, 1, 3).contiguous().requires_grad_(True) for t in (q, k, v)]
    mask = O.build_mask(q.shape[1], k.shape[1], sep)
    o = O.standard_attention(qr, kr, vr, mask, drop)
    if dout is not None:
        o.backward(dout.float().permute(0, 2, 1, 3))
        return o.permute(0, 2, 1, 3), [t.grad.permute(0, 2, 1, 3) for t in (qr, kr, vr)]
    return o.permute(0, 2, 1, 3), None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,H,s_q,s_k,sep", [(2, 2, 40, 40, 0), (1, 3, 200, 200, 0), (2, 1, 24, 40, 5), (1, 2, 321, 321, 0),
                                             (1, 1, 1, 77, 0), (1, 2, 130, 130, 37)])
def test_attention_fwd_bwd(ops, dtype, b, H, s_q, s_k, sep):
    g = torch.Generator().manual_seed(s_q * 3 + s_k)
    # q/k/v as strided views of one [b, s, 3*H*64] buffer, exactly how the QKV GEMM output is consumed
    qkv = rnd((b, s_k, 3 * H * 64), dtype, g)
    q = qkv[:, s_k - s_q:, 0:H * 64].reshape(b, s_q, H, 64)
    k = qkv[:, :, H * 64:2 * H * 64].reshape(b, s_k, H, 64)
    v = qkv[:, :, 2 * H * 64:].reshape(b, s_k, H, 64)
    dout = rnd((b, s_q, H, 64), dtype, g)
    o_ref, grads = _attn_ref(q, k, v, sep, None, dout)
    qkv_d = dev(qkv)
    qd = qkv_d[:, s_k - s_q:, 0:H * 64].view(b, s_q, H, 64)
    kd = qkv_d[:, :, H * 64:2 * H * 64].view(b, s_k, H, 64)
    vd = qkv_d[:, :, 2 * H * 64:].view(b, s_k, H, 64)
    o, lse = ops.attention_fwd(qd, kd, vd, sep=sep)
    assert rel(o, o_ref) < TOL[dtype]
    dq, dk, dv = ops.attention_bwd(dev(dout), qd, kd, vd, o, lse, sep=sep)
    for name, got, want in zip("qkv", (dq, dk, dv), grads):
        assert rel(got, want) < TOL[dtype] * 2, name


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_dropout_mask_replay(ops, dtype):
    g = torch.Generator().manual_seed(21)
    b, H, s = 2, 2, 96
    q, k, v, dout = [rnd((b, s, H, 64), dtype, g) for _ in range(4)]
    drop = torch.from_numpy(O.attention_keep_mask(b, H, s, s, 0.1, 31, 9))
    o_ref, grads = _attn_ref(q, k, v, 0, drop, dout)
    qd, kd, vd = dev(q), dev(k), dev(v)
    o, lse = ops.attention_fwd(qd, kd, vd, dropout=(0.1, 31, 9))
    assert rel(o, o_ref) < TOL[dtype]
    dq, dk, dv = ops.attention_bwd(dev(dout), qd, kd, vd, o, lse, dropout=(0.1, 31, 9))
    for name, got, want in zip("qkv", (dq, dk, dv), grads):
        assert rel(got, want) < TOL[dtype] * 2, name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,H,s_q,s_k,sep", [(2, 3, 1088, 1088, 0), (1, 2, 320, 1088, 70)])
def test_attention_dropout_at_the_bench_length_vs_oracle(ops, dtype, b, H, s_q, s_k, sep):
    """Attention dropout (p = 0.1, what bench.py runs) against the oracle's mask at the BASELINE length: 1088 x 1088
    is 17 key blocks per query tile -- the per-row keys published by the dQ kernel, the Weyl step per 4-key group and the
    quad-shared masks of the dK/dV kernel all have to line up across blocks (round 2 checked one block, s = 96) -- and a
    `sep` + memory shape (320 queries over 1088 keys, the first 70 + 768 fully visible).  Forward and dQ / dK / dV,
    q / k / v as strided views of the QKV buffer as in the layer (mpu/sparse_transformer.py:652-673)."""
    g = torch.Generator().manual_seed(s_q + 7 * s_k)
    qkv = rnd((b, s_k, 3 * H * 64), dtype, g)
    q = qkv[:, s_k - s_q:, 0:H * 64].reshape(b, s_q, H, 64)
    k = qkv[:, :, H * 64:2 * H * 64].reshape(b, s_k, H, 64)
    v = qkv[:, :, 2 * H * 64:].reshape(b, s_k, H, 64)
    dout = rnd((b, s_q, H, 64), dtype, g)
    drop = torch.from_numpy(O.attention_keep_mask(b, H, s_q, s_k, 0.1, 77, 5))
    o_ref, grads = _attn_ref(q, k, v, sep, drop, dout)
    qkv_d = dev(qkv)
    qd = qkv_d[:, s_k - s_q:, 0:H * 64].view(b, s_q, H, 64)
    kd = qkv_d[:, :, H * 64:2 * H * 64].view(b, s_k, H, 64)
    vd = qkv_d[:, :, 2 * H * 64:].view(b, s_k, H, 64)
    o, lse = ops.attention_fwd(qd, kd, vd, sep=sep, dropout=(0.1, 77, 5))
    assert rel(o, o_ref) < TOL[dtype]
    # a wrong mask on a single key block is a ~10 % error of that block's rows: look at the worst 64-row slab too
    worst = max(rel(o[:, i:i + 64], o_ref[:, i:i + 64]) for i in range(0, s_q, 64))
    assert worst < TOL[dtype] * 2, worst
    dq, dk, dv = ops.attention_bwd(dev(dout), qd, kd, vd, o, lse, sep=sep, dropout=(0.1, 77, 5))
    for name, got, want in zip("qkv", (dq, dk, dv), grads):
        assert rel(got, want) < TOL[dtype] * 2, name
        n = got.shape[1]
        worst = max(rel(got[:, i:i + 64], want[:, i:i + 64]) for i in range(0, n, 64))
        assert worst < TOL[dtype] * 4, (name, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,H,s_q,s_k,sep", [(2, 3, 1088, 1088, 0), (1, 2, 320, 1088, 70), (3, 2, 255, 255, 0), (1, 1, 96, 160, 0)])
def test_attention_stored_keep_bits_equal_the_regenerated_mask(ops, dtype, b, H, s_q, s_k, sep):
    """The forward kernel stores its dropout keep decisions (cogv_attn_desc.keep_bits: the reference keeps the dropout mask
    of mpu/sparse_transformer.py:667-669 for autograd) and the backward kernels read them instead of regenerating the
    draws.  The stored form must reproduce the regenerating form BIT FOR BIT -- forward output and dQ / dK / dV -- at the
    bench length (17 key blocks), a `sep` + memory shape, the ragged cfg 1 length (255) and a short memory shape; the
    regenerating form itself is pinned to the oracle's mask by the two tests above.  The bit buffer starts as 0xFF / 0x00
    garbage: words the forward pass does not write (blocks above the diagonal) must not matter."""
    g = torch.Generator().manual_seed(3 * s_q + s_k)
    qkv = dev(rnd((b, s_k, 3 * H * 64), dtype, g))
    q = qkv[:, s_k - s_q:, 0:H * 64].view(b, s_q, H, 64)
    k = qkv[:, :, H * 64:2 * H * 64].view(b, s_k, H, 64)
    v = qkv[:, :, 2 * H * 64:].view(b, s_k, H, 64)
    dout = dev(rnd((b, s_q, H, 64), dtype, g))
    drop = (0.1, 77, 5)
    o0, lse0 = ops.attention_fwd(q, k, v, sep=sep, dropout=drop)
    ref = ops.attention_bwd(dout, q, k, v, o0, lse0, sep=sep, dropout=drop)
    for fill in (0xFF, 0x00):
        torch.cuda.synchronize()
        junk = torch.full((512 << 20,), fill, dtype=torch.uint8, device="cuda")      # the allocator hands this memory back below
        del junk
        o1, lse1, bits = ops.attention_fwd(q, k, v, sep=sep, dropout=drop, keep_bits=True)
        assert bits is not None and bits.dtype == torch.uint8
        assert torch.equal(o1, o0) and torch.equal(lse1, lse0)
        got = ops.attention_bwd(dout, q, k, v, o1, lse1, sep=sep, dropout=drop, keep_bits=bits)
        for name, a_, b_ in zip("qkv", got, ref):
            assert torch.equal(a_, b_), (name, fill, rel(a_, b_))
    # the fraction of kept scores among the words the forward pass wrote: 1 - p
    w = bits.view(torch.int32).view(b, H, (s_k + 63) // 64, 2, s_q)
    first = w[:, :, 0, :, s_q - 1].reshape(-1)                  # key block 0 is visible to the last query in every shape here
    ones = sum(bin(int(x) & 0xFFFFFFFF).count("1") for x in first.tolist())
    assert abs(ones / (32.0 * first.numel()) - 0.9) < 0.08


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["per_sample_binary", "shared_fractional", "memory_keys_with_dropout"])
def test_attention_arbitrary_mask_tensor_vs_oracle(ops, dtype, kind):
    """mpu/sparse_transformer.py:661-663 multiplies the scores by WHATEVER mask it is given:  S * M - 10000 * (1 - M).  The
    kernels' general-mask path (cogv_attn_desc.mask) against the oracle, forward and dQ / dK / dV: a different random binary
    mask per sample ([b, 1, s, s]: the round-3 verdict's missing item), one NON-binary mask shared by the batch (values 0,
    0.25, 1: the formula is linear in M, the kernels implement it, not a visibility bit), and more keys than queries with
    attention dropout on top.  Ragged sizes (no multiple of 32 / 64)."""
    g = torch.Generator().manual_seed(len(kind))
    if kind == "per_sample_binary":
        b, H, s_q, s_k, drop = 3, 2, 150, 150, None
        m = (torch.rand(b, 1, s_q, s_k, generator=g) < 0.6).float()
        m[..., 0] = 1.0                                   # no empty row
    elif kind == "shared_fractional":
        b, H, s_q, s_k, drop = 2, 2, 97, 97, None
        m = torch.tensor([0.0, 0.25, 1.0])[torch.randint(0, 3, (1, 1, s_q, s_k), generator=g)]
        m[..., 0] = 1.0
    else:
        b, H, s_q, s_k, drop = 2, 1, 70, 200, (0.1, 41, 3)
        m = (torch.rand(b, 1, s_q, s_k, generator=g) < 0.5).float()
        m[..., 0] = 1.0
    q, dout = rnd((b, s_q, H, 64), dtype, g), rnd((b, s_q, H, 64), dtype, g)
    k, v = rnd((b, s_k, H, 64), dtype, g), rnd((b, s_k, H, 64), dtype, g)
    keep = None if drop is None else torch.from_numpy(O.attention_keep_mask(b, H, s_q, s_k, *drop))
    qr, kr, vr = [t.float().permute(0, 2, 1, 3).contiguous().requires_grad_(True) for t in (q, k, v)]
    o_ref = O.standard_attention(qr, kr, vr, m, keep)
    o_ref.backward(dout.float().permute(0, 2, 1, 3))
    grads = [t.grad.permute(0, 2, 1, 3) for t in (qr, kr, vr)]
    md = dev(m.reshape(-1, s_q, s_k).to(dtype))
    qd, kd, vd = dev(q), dev(k), dev(v)
    o, lse = ops.attention_fwd(qd, kd, vd, dropout=drop, mask=md)
    assert rel(o, o_ref.permute(0, 2, 1, 3)) < TOL[dtype]
    dq, dk, dv = ops.attention_bwd(dev(dout), qd, kd, vd, o, lse, dropout=drop, mask=md)
    for name, got, want in zip("qkv", (dq, dk, dv), grads):
        assert rel(got, want) < TOL[dtype] * 2, (name, rel(got, want))


def test_standard_attention_module_surface_takes_any_mask(ops):
    """functional.standard_attention (the drop-in of mpu/sparse_transformer.py:652-673, tensors [b, np, s, hn]): a left-to-right
    mask tensor is recognised and takes the `sep` kernels; any other tensor goes to the general-mask path -- both through
    autograd, against the oracle."""
    from cogview_amd import functional as F_
    g = torch.Generator().manual_seed(4)
    b, H, s = 2, 2, 72
    for general in (False, True):
        m = O.build_mask(s, s) if not general else (torch.rand(b, 1, s, s, generator=g) < 0.7).float()
        if general:
            m[..., 0] = 1.0
        q, k, v = [rnd((b, H, s, 64), torch.float16, g) for _ in range(3)]
        dout = rnd((b, H, s, 64), torch.float16, g)
        qd, kd, vd = [dev(t).requires_grad_(True) for t in (q, k, v)]
        md = dev(m.half())
        assert (F_.mask_to_sep(md, s, s) is None) == general
        out = F_.standard_attention(qd, kd, vd, md)
        out.backward(dev(dout))
        qr, kr, vr = [t.float().requires_grad_(True) for t in (q, k, v)]
        ref = O.standard_attention(qr, kr, vr, m)
        ref.backward(dout.float())
        assert rel(out, ref) < TOL[torch.float16]
        for got, want in ((qd.grad, qr.grad), (kd.grad, kr.grad), (vd.grad, vr.grad)):
            assert rel(got, want) < TOL[torch.float16] * 2


def test_attention_full_length_properties(ops):
    """s = 1088 (BASELINE sequence): causal property -- output at position i must not change when
    later keys/values change; checked bit-exactly."""
    g = torch.Generator().manual_seed(5)
    b, H, s = 1, 2, 1088
    q, k, v = [dev(rnd((b, s, H, 64), torch.float16, g)) for _ in range(3)]
    o1, _ = ops.attention_fwd(q, k, v)
    k2, v2 = k.clone(), v.clone()
    k2[:, 600:] = 7.0
    v2[:, 600:] = -3.0
    o2, _ = ops.attention_fwd(q, k2, v2)
    assert torch.equal(o1[:, :600], o2[:, :600])
    assert not torch.equal(o1[:, 600:], o2[:, 600:])
    assert torch.isfinite(o1.float()).all()


# ------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("dtype", DTYPES)
def test_embedding_fwd_bwd(ops, dtype):
    g = torch.Generator().manual_seed(6)
    V, P, h, b, s = 96, 48, 128, 2, 40
    table, pos_table = rnd((V, h), dtype, g), rnd((P, h), dtype, g)
    ids = torch.randint(0, 128, (b, s), generator=g)          # some ids outside the shard [16, 112)
    pos = torch.arange(s).unsqueeze(0).expand(b, -1)
    vs = 16
    inside = (ids >= vs) & (ids < vs + V)
    word = torch.where(inside.unsqueeze(-1), table.float()[(ids - vs).clamp(0, V - 1)], torch.zeros(1))
    ref = (word + pos_table.float()[pos]).to(dtype).float()
    mask = torch.from_numpy(O.dropout_keep_mask(b * s * h, 0.1, 3, 1)).view(b, s, h)
    slot = ops.new_absmax_slot(torch.device("cuda"))
    out = ops.embedding_fwd(dev(ids), dev(table), vs, dev(pos), dev(pos_table), dropout=(0.1, 3, 1), absmax_out=slot)
    assert rel(out, ref * mask) < TOL[dtype]
    assert slot.item() == out.float().abs().max().item()
    dout = rnd((b, s, h), dtype, g)
    dt = torch.zeros((V, h), dtype=dtype, device="cuda")
    dp = torch.zeros((P, h), dtype=dtype, device="cuda")
    ops.embedding_bwd(dev(dout), dev(ids), dt, vs, dev(pos), dp, dropout=(0.1, 3, 1))
    dm = dout.float() * mask
    rt = torch.zeros(V, h).index_add_(0, (ids - vs).clamp(0, V - 1).view(-1), (dm * inside.unsqueeze(-1)).view(-1, h))
    rp = torch.zeros(P, h).index_add_(0, pos.reshape(-1), dm.view(-1, h))
    assert rel(dt, rt) < TOL[dtype] * 3
    assert rel(dp, rp) < TOL[dtype] * 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_elementwise(ops, dtype):
    g = torch.Generator().manual_seed(8)
    x, dy = rnd((33, 256), dtype, g, 2.0), rnd((33, 256), dtype, g)
    assert rel(ops.gelu_fwd(dev(x)), O.gelu(x.float())) < TOL[dtype]
    xr = x.float().requires_grad_(True)
    O.gelu(xr).backward(dy.float())
    assert rel(ops.gelu_bwd(dev(dy), dev(x)), xr.grad) < TOL[dtype]
    mask = torch.from_numpy(O.dropout_keep_mask(x.numel(), 0.25, 1, 2)).view_as(x)
    assert rel(ops.dropout(dev(x), 0.25, 1, 2), x.float() * mask) < TOL[dtype]
    assert rel(ops.add(dev(x), dev(dy)), x.float() + dy.float()) < TOL[dtype]
    assert rel(ops.colsum(dev(x)), x.float().sum(0)) < TOL[dtype]
    big = rnd((2000, 1024), dtype, g)
    assert rel(ops.colsum(dev(big)), big.float().sum(0)) < TOL[dtype]


# ------------------------------------------------------------------------------------------------ CE
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows,V", [(14, 96), (80, 58240), (5, 29184)])
def test_cross_entropy(ops, dtype, rows, V):
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(rows, V, generator=g) * 4).to(dtype)
    tgt = torch.randint(0, V, (rows,), generator=g)
    lr = logits.float().requires_grad_(True)
    ce = O.vocab_parallel_cross_entropy(lr, tgt)
    w = torch.rand(rows, generator=g)
    (ce * w).sum().backward()
    rowmax, sumexp, pred, loss = ops.ce_fwd(dev(logits), dev(tgt), 0)
    assert rel(loss, ce) < 1e-5
    d = ops.ce_bwd(dev(logits), dev(tgt), 0, rowmax, sumexp, dev(w))
    tol = 1e-5 if dtype == torch.float32 else TOL[dtype]
    assert rel(d, lr.grad) < tol
    # two-shard statistics combine to the same loss (plays the 3 all-reduces of mpu/cross_entropy.py)
    half = V // 2
    if half % 8 == 0:
        a = ops.ce_fwd(dev(logits[:, :half].contiguous()), dev(tgt), 0, want_loss=False)
        b = ops.ce_fwd(dev(logits[:, half:].contiguous()), dev(tgt), half, want_loss=False)
        gm = torch.maximum(a[0], b[0])
        gs = a[1] * torch.exp(a[0] - gm) + b[1] * torch.exp(b[0] - gm)
        loss2 = torch.log(gs) + gm - (a[2] + b[2])
        assert rel(loss2, ce) < 1e-5


# ------------------------------------------------------------------------------------------------ optimizer
@pytest.mark.parametrize("dtype", DTYPES)
def test_grad_stats_and_adamw(ops, dtype):
    g = torch.Generator().manual_seed(12)
    sizes = [1000, 24, 4096, 130, 70000]
    offs, o = [], 0
    for s in sizes:
        offs.append(o)
        o += (s + 127) // 128 * 128
    total = o
    p32 = torch.zeros(total)
    grads = torch.zeros(total)
    for s, of in zip(sizes, offs):
        p32[of:of + s] = torch.randn(s, generator=g)
        grads[of:of + s] = torch.randn(s, generator=g) * 64.0
    p16 = p32.to(dtype)
    g16 = grads.to(dtype)
    # chunk table: chunks of <= 32768 elements, groups: tensors 0,2,4 decay (group 0), 1,3 no decay (group 1)
    cs, cl, cg, cn = [], [], [], []
    for i, (s, of) in enumerate(zip(sizes, offs)):
        for c0 in range(0, s, 32768):
            cs.append(of + c0)
            cl.append(min(32768, s - c0))
            cg.append(i % 2)
            cn.append(0 if i == 3 else 1)          # tensor 3 excluded from the norm (MP dedup)
    D = "cuda"
    cs_t, cl_t = torch.tensor(cs, dtype=torch.int64, device=D), torch.tensor(cl, dtype=torch.int32, device=D)
    cg_t, cn_t = torch.tensor(cg, dtype=torch.uint8, device=D), torch.tensor(cn, dtype=torch.uint8, device=D)
    stats = torch.zeros(2, dtype=torch.float64, device=D)
    ops.grad_stats(dev(g16), cs_t, cl_t, cn_t, stats)
    ref_sq = sum(float((g16[of:of + s].double() ** 2).sum()) for i, (s, of) in enumerate(zip(sizes, offs)) if i != 3)
    assert abs(stats[0].item() - ref_sq) < 1e-5 * ref_sq and stats[1].item() == 0.0
    # oracle: unscale by 1/64, clip to 1.0, AdamW with per-group weight decay, 2 steps
    lr, wd, scale, max_norm = 1e-2, 0.1, 64.0, 1.0
    master = p16.float().clone()
    m, v = torch.zeros(total), torch.zeros(total)
    pd, gd = dev(p16.clone()), dev(g16)
    md, ed, vd = dev(master.clone()), dev(m.clone()), dev(v.clone())
    for step in (1, 2):
        gs = [g16[of:of + s].float() / scale for s, of in zip(sizes, offs)]
        norm = math.sqrt(sum(float(x.double().norm() ** 2) for i, x in enumerate(gs) if i != 3))
        coef = max_norm / (norm + 1e-6)
        for i, (s, of) in enumerate(zip(sizes, offs)):
            gi = gs[i] * coef if coef < 1 else gs[i]
            O.adamw_step(master[of:of + s], gi, m[of:of + s], v[of:of + s], step, lr, weight_decay=wd if i % 2 == 0 else 0.0)
        stats.zero_()
        ops.grad_stats(gd, cs_t, cl_t, cn_t, stats)
        ops.adamw_step(pd, gd, md, ed, vd, cs_t, cl_t, cg_t, [lr, lr], [wd, 0.0], 0.9, 0.999, 1e-8, step,
                       inv_loss_scale=1.0 / scale, max_grad_norm=max_norm, stats=stats)
    assert rel(md, master) < 1e-5
    assert rel(ed, m) < 1e-5 and rel(vd, v) < 1e-5
    assert torch.equal(pd.cpu(), md.cpu().to(dtype))
    # overflow: an inf anywhere flags the step and the kernel leaves everything untouched
    gbad = g16.clone()
    gbad[offs[2] + 5] = float("inf")
    stats.zero_()
    ops.grad_stats(dev(gbad), cs_t, cl_t, cn_t, stats)
    assert stats[1].item() == 1.0
    before = md.clone()
    ops.adamw_step(pd, dev(gbad), md, ed, vd, cs_t, cl_t, cg_t, [lr, lr], [wd, 0.0], 0.9, 0.999, 1e-8, 3,
                   inv_loss_scale=1.0 / scale, max_grad_norm=max_norm, stats=stats)
    assert torch.equal(before, md)


def test_grad_stats_is_run_to_run_deterministic(ops):
    """The global sum of squares is per-workgroup partials summed in workgroup order (no floating-point atomics): identical
    bits on every run, also with far more chunks than workgroups, and stats[0] accumulates across calls."""
    g = torch.Generator().manual_seed(99)
    n = 5000 * 4096 + 1234                                 # 5001 chunks > 2048 workgroups
    grads = dev((torch.randn(n, generator=g) * 3.0).half())
    cs = torch.arange(0, n, 4096, dtype=torch.int64)
    cl = torch.full((len(cs),), 4096, dtype=torch.int32)
    cl[-1] = n - int(cs[-1])
    cn = torch.ones(len(cs), dtype=torch.uint8)
    cs, cl, cn = dev(cs), dev(cl), dev(cn)
    outs = []
    for _ in range(5):
        stats = torch.zeros(2, dtype=torch.float64, device="cuda")
        ops.grad_stats(grads, cs, cl, cn, stats)
        outs.append(stats.clone())
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    ref = float((grads.double() ** 2).sum())
    assert abs(outs[0][0].item() - ref) < 1e-6 * ref and outs[0][1].item() == 0.0
    ops.grad_stats(grads, cs, cl, cn, stats)               # second call on the same stats: accumulates
    assert stats[0].item() == 2.0 * outs[0][0].item()


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_bwd_fused_qkv_bias_grad(ops, dtype):
    """colsum_out of cogv_attention_bwd == column sums of the stored dq | dk | dv (bias gradient of the QKV linear)."""
    g = torch.Generator().manual_seed(5)
    b, s, H = 2, 300, 3
    qkv = dev(rnd((b, s, 3 * H * 64), dtype, g))
    q, k, v = [qkv[:, :, i * H * 64:(i + 1) * H * 64].view(b, s, H, 64) for i in range(3)]
    do = dev(rnd((b, s, H, 64), dtype, g))
    o, lse = ops.attention_fwd(q, k, v, dropout=(0.1, 3, 4))
    prev = rnd((3 * H * 64,), dtype, g)
    fused = dev(prev.clone())
    dq, dk, dv = ops.attention_bwd(do, q, k, v, o, lse, dropout=(0.1, 3, 4), colsum_out=fused)
    dq2, dk2, dv2 = ops.attention_bwd(do, q, k, v, o, lse, dropout=(0.1, 3, 4))
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2)
    expect = torch.cat([t.float().reshape(-1, H * 64).sum(0) for t in (dq, dk, dv)]).cpu() + prev.float()
    assert rel(fused, expect) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_sparse_attention_inference_vs_reference_golden(ops, dtype, golden_dir):
    """Gathered-key forward (sparse_attention_inference, mpu/sparse_transformer.py:727-750) against the REFERENCE's
    own output (tests/golden/sparse_attention.npz) and, at a longer gathered length with several queries, the oracle."""
    import numpy as np
    from cogview_amd import mpu
    F_ = mpu.transformer
    z = np.load(os.path.join(golden_dir, "sparse_attention.npz"))
    t = {k: torch.from_numpy(z[k]) for k in z.files}
    sq, sk = [int(x) for x in t["inf_cfg"]]
    q = t["q"][:, :, sk - sq:sk].to(dtype)
    k, v = t["k"][:, :, :sk].to(dtype), t["v"][:, :, :sk].to(dtype)
    with torch.no_grad():
        out = F_.sparse_attention_inference(dev(q), dev(k), dev(v), dev(t["pw_idx"]))
    ref = O.sparse_attention_inference(q.float(), k.float(), v.float(), t["pw_idx"])
    assert rel(out, t["inf_ctx"]) < 3 * TOL[dtype]           # golden was computed from unrounded inputs
    assert rel(out, ref) < TOL[dtype]
    g = torch.Generator().manual_seed(9)
    b, nh, s, n, sq = 2, 3, 700, 333, 5
    q, k, v = [rnd((b, nh, s, 64), dtype, g) for _ in range(3)]
    idx = torch.stack([torch.cat((torch.randperm(s - sq, generator=g)[:n - sq].sort().values, torch.arange(s - sq, s)))
                       for _ in range(b)])
    with torch.no_grad():
        out = F_.sparse_attention_inference(dev(q[:, :, -sq:]), dev(k), dev(v), dev(idx))
    ref = O.sparse_attention_inference(q[:, :, -sq:].float(), k.float(), v.float(), idx)
    assert rel(out, ref) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_sparse_attention_training_form_forward(ops, dtype):
    """Forward of the sparse TRAINING form (pivots + window, joint softmax; mpu/sparse_transformer.py:675-725) computed
    in slot space by the gathered attention kernel, against the oracle restatement (itself pinned to the reference)."""
    from cogview_amd import mpu                      # (importing the package first avoids the functional <-> mpu cycle)
    from cogview_amd import functional as F_
    g = torch.Generator().manual_seed(21)
    b, nh, w, times, n_piv = 2, 3, 128, 2, 40
    s = 4 * w
    q, k, v = [rnd((b, nh, s, 64), dtype, g) for _ in range(3)]
    pivot_idx = torch.stack([torch.cat((torch.arange(7), 7 + torch.randperm(s - 7, generator=g)[:n_piv - 7])) for _ in range(b)])
    rmask = O.sparse_rmask(s, w, times)
    pam = rmask.expand(b, s, s).gather(-1, pivot_idx.unsqueeze(1).expand(b, s, n_piv))
    ref = O.sparse_attention(q.float(), k.float(), v.float(), pivot_idx, pam, w, times)
    tab = F_.sparse_slot_table(dev(pivot_idx), s, w, times)
    qd, kd, vd = [dev(t).permute(0, 2, 1, 3).contiguous() for t in (q, k, v)]          # [b, s, H, 64]
    out, _ = ops.attention_fwd(qd, kd, vd, kv_index=tab, sparse=(w, n_piv, math.log(s // n_piv)))
    assert rel(out.permute(0, 2, 1, 3), ref) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("times,n_piv", [(2, 40), (3, 72)])
def test_sparse_attention_training_form_backward(ops, dtype, times, n_piv):
    """mpu.sparse_attention (drop-in for mpu/sparse_transformer.py:675-725) forward + input gradients against the
    oracle restatement's autograd: dQ gathers keys through the slot table, dK/dV are computed per (batch, query block)
    in slot space and folded back onto the keys by cogv_sparse_slot_reduce (window copies + pivot copies)."""
    from cogview_amd import mpu
    g = torch.Generator().manual_seed(33 + times)
    b, nh, w = 2, 3, 128
    s = 5 * w
    q, k, v, dout = [rnd((b, nh, s, 64), dtype, g) for _ in range(4)]
    pivot_idx = torch.stack([torch.cat((torch.arange(9), 9 + torch.randperm(s - 9, generator=g)[:n_piv - 9])) for _ in range(b)])
    pam = O.sparse_rmask(s, w, times).expand(b, s, s).gather(-1, pivot_idx.unsqueeze(1).expand(b, s, n_piv))
    qf, kf, vf = [t.float().requires_grad_(True) for t in (q, k, v)]
    ref = O.sparse_attention(qf, kf, vf, pivot_idx, pam, w, times)
    ref.backward(dout.float())
    qd, kd, vd = [dev(t).requires_grad_(True) for t in (q, k, v)]
    out = mpu.transformer.sparse_attention(qd, kd, vd, dev(pivot_idx), dev(pam), w, times)
    out.backward(dev(dout))
    assert rel(out, ref) < TOL[dtype]
    for name, a, r in (("dq", qd.grad, qf.grad), ("dk", kd.grad, kf.grad), ("dv", vd.grad, vf.grad)):
        e = rel(a, r)
        assert e < 2 * TOL[dtype], f"{name}: {e}"


def test_sparse_attention_training_form_dropout_adjoint(ops):
    """With attention dropout the context is still linear in V for a fixed mask, so <dO, O(V)> == <dV, V> holds iff
    the backward kernels regenerate exactly the forward's keep mask in slot space (row, slot counters)."""
    from cogview_amd import mpu
    from cogview_amd import functional as F_
    g = torch.Generator().manual_seed(5)
    b, nh, w, times, n_piv = 1, 2, 128, 2, 24
    s = 3 * w
    q, k, v, dout = [dev(rnd((b, s, nh, 64), torch.float16, g)) for _ in range(4)]
    pivot_idx = dev(torch.stack([torch.randperm(s, generator=g)[:n_piv] for _ in range(b)]))
    tab, inv = F_.sparse_pivot_plan(pivot_idx, s, w, times)
    sp = (w, n_piv, math.log(s // n_piv))
    drop = (0.25, 1234, 77)
    o, lse = ops.attention_fwd(q, k, v, dropout=drop, kv_index=tab, sparse=sp)
    o0, _ = ops.attention_fwd(q, k, v, kv_index=tab, sparse=sp)
    assert 0.2 < rel(o, o0) < 2.0                   # dropout really happened
    dq, dk, dv = ops.sparse_attention_bwd(dout, q, k, v, o, lse, tab, sp, inv, times, dropout=drop)
    lhs = (dout.double() * o.double()).sum().item()
    rhs = (dv.double() * v.double()).sum().item()
    assert abs(lhs - rhs) < 5e-3 * (dout.double().norm() * o.double().norm()).item(), (lhs, rhs)
    # the dropout-free gradient differs (sanity: the identity above is not trivially true)
    _, _, dv0 = ops.sparse_attention_bwd(dout, q, k, v, o0, lse, tab, sp, inv, times)
    assert rel(dv0, dv) > 0.1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,H,cap,pos", [(1, 2, 128, 0), (2, 3, 300, 127), (2, 3, 300, 128), (1, 40, 1152, 1024), (3, 2, 256, 255)])
def test_attention_decode_step(ops, dtype, b, H, cap, pos):
    """cogv_attention_decode: one query token against a fixed-capacity cache (keys split over workgroups, last arriver
    combines, cache append fused) == the oracle's standard_attention (mpu/sparse_transformer.py:652-673) of that query
    over slots [0, pos] with the new token's key / value in slot pos; the cache afterwards holds them; a second launch
    (re-armed tickets, as in a graph replay) gives the same bits."""
    g = torch.Generator().manual_seed(cap + pos)
    hp = H * 64
    cache = rnd((b, cap, 2 * hp), dtype, g)
    qkv = rnd((b, 1, 3 * hp), dtype, g)
    cache_d, qkv_d = dev(cache.clone()), dev(qkv)
    pos_d = torch.tensor([pos], dtype=torch.int64, device="cuda")
    out = ops.attention_decode(qkv_d, cache_d, pos_d, H)
    want_cache = cache.clone()
    want_cache[:, pos, :hp] = qkv[:, 0, hp:2 * hp]
    want_cache[:, pos, hp:] = qkv[:, 0, 2 * hp:]
    assert torch.equal(cache_d.cpu(), want_cache), "the new key / value must land in slot pos and nothing else may change"
    q = qkv[:, :, :hp].float().view(b, 1, H, 64).permute(0, 2, 1, 3)
    k = want_cache[:, :pos + 1, :hp].float().view(b, pos + 1, H, 64).permute(0, 2, 1, 3)
    v = want_cache[:, :pos + 1, hp:].float().view(b, pos + 1, H, 64).permute(0, 2, 1, 3)
    ref = O.standard_attention(q, k, v, torch.ones(1, 1, 1, pos + 1)).permute(0, 2, 1, 3).reshape(b, 1, hp)
    assert rel(out, ref) < TOL[dtype]
    again = ops.attention_decode(qkv_d, cache_d, pos_d, H)
    assert torch.equal(out, again)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,H,cap,pos,N", [(1, 8, 256, 100, 512), (4, 40, 1152, 1024, 2560), (8, 16, 384, 383, 1024), (2, 8, 128, 0, 64)])
def test_attention_output_projection_with_combine_prologue(ops, dtype, b, H, cap, pos, N):
    """cogv_gemv_attn: the attention-output projection of a decode step whose input is COMBINED from the decode attention's
    key-split partials inside the kernel (round 3: one launch per layer less) == the two-launch form of the same library
    (cogv_attention_decode with its combine kernel, then the skinny-M GEMV) and the oracle's definition
    (mpu/sparse_transformer.py:652-673, :163-166): dense(standard_attention(q, K[0..pos], V[0..pos])) with bias; abs-max slot."""
    g = torch.Generator().manual_seed(cap + pos + N)
    hp = H * 64
    cache, qkv = rnd((b, cap, 2 * hp), dtype, g), rnd((b, 1, 3 * hp), dtype, g)
    w, bias = rnd((N, hp), dtype, g, 0.05), rnd((N,), dtype, g)
    pos_d = torch.tensor([pos], dtype=torch.int64, device="cuda")
    c1, c2 = dev(cache.clone()), dev(cache.clone())
    att = ops.attention_decode(dev(qkv), c1, pos_d, H)
    slot_ref = ops.new_absmax_slot(att.device)
    ref2 = ops.gemm(att.view(b, hp), dev(w), bias=dev(bias), absmax=slot_ref)
    parts = ops.attention_decode(dev(qkv), c2, pos_d, H, combine=False)
    assert torch.equal(c1, c2)                                   # the cache append does not depend on the form
    slot = ops.new_absmax_slot(att.device)
    out = ops.gemv_attn(parts, b, H, cap, dev(w), bias=dev(bias), absmax=slot)
    # same arithmetic in the same association as the combine kernel + the skinny-M GEMV: the two forms agree bit for bit
    # (a captured decode graph uses the two-launch form, the eager step this one)
    assert out.shape == (b, N) and torch.equal(out, ref2)
    assert slot.item() == slot_ref.item()
    want_cache = cache.clone()
    want_cache[:, pos, :hp] = qkv[:, 0, hp:2 * hp]
    want_cache[:, pos, hp:] = qkv[:, 0, 2 * hp:]
    q = qkv[:, :, :hp].float().view(b, 1, H, 64).permute(0, 2, 1, 3)
    k = want_cache[:, :pos + 1, :hp].float().view(b, pos + 1, H, 64).permute(0, 2, 1, 3)
    v = want_cache[:, :pos + 1, hp:].float().view(b, pos + 1, H, 64).permute(0, 2, 1, 3)
    a_ref = O.standard_attention(q, k, v, torch.ones(1, 1, 1, pos + 1)).permute(0, 2, 1, 3).reshape(b, hp)
    ref = O.linear(a_ref.to(dtype).float(), w.float(), bias.float())
    assert rel(out, ref) < TOL[dtype]
    assert torch.equal(out, ops.gemv_attn(parts, b, H, cap, dev(w), bias=dev(bias)))      # replayable: no hidden state


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,N,post,gelu", [(1, 512, 768, False, False), (3, 1024, 512, True, True), (8, 2560, 1024, True, False),
                                              (2, 4096, 256, True, True), (5, 512, 64, False, True), (1, 2560, 7680, True, False),
                                              (2, 2560, 24, False, True), (4, 1536, 136, True, False), (1, 1024, 40, True, True)])
def test_gemv_with_layernorm_prologue(ops, dtype, M, K, N, post, gelu):
    """cogv_gemv_ln == the unfused chain of the same library (Sandwich-LN kernels, then the GEMV with the same epilogue)
    and the oracle's definition (mpu/sparse_transformer.py:326-341): t = residual + LN_post(z), x_in = LN_pre(t),
    out = [gelu](x_in W^T + b); every row count bucket of the kernel (1, 2, 4, 8 with padding rows), the residual stream
    written once, the output abs-max slot."""
    g = torch.Generator().manual_seed(M * 100 + K + N)
    z, res = rnd((M, K), dtype, g, 3.0), rnd((M, K), dtype, g)
    w, bias = rnd((N, K), dtype, g, 0.05), rnd((N,), dtype, g)
    gp, bp = (1.0 + 0.1 * torch.randn(K, generator=g)).to(dtype), (0.1 * torch.randn(K, generator=g)).to(dtype)
    gn, bn = (1.0 + 0.1 * torch.randn(K, generator=g)).to(dtype), (0.1 * torch.randn(K, generator=g)).to(dtype)
    eps = 1e-5
    zd, resd = dev(z), dev(res)
    zmax = ops.absmax(zd)
    # unfused chain on the GPU
    if post:
        slot_t = ops.new_absmax_slot(zd.device)
        t_ref, _, _ = ops.sandwich_ln_fwd(zd, dev(gp), dev(bp), eps, zmax, residual=resd, absmax_out=slot_t, save_stats=False)
    else:
        t_ref, slot_t = zd, zmax
    x_ref, _, _ = ops.sandwich_ln_fwd(t_ref, dev(gn), dev(bn), eps, slot_t, save_stats=False)
    slot_ref = ops.new_absmax_slot(zd.device)
    out_ref = ops.gemm(x_ref, dev(w), bias=dev(bias), gelu=gelu, absmax=slot_ref)
    slot = ops.new_absmax_slot(zd.device)
    out, t = ops.gemv_ln(zd, dev(w), dev(bias), dev(gn), dev(bn), eps, z_absmax=zmax, post=(dev(gp), dev(bp)) if post else None,
                         residual=resd if post else None, want_t=post, gelu=gelu, absmax=slot)
    if post:
        assert torch.equal(t, t_ref), "the residual stream written by workgroup 0 must equal the LayerNorm kernel's"
        # max|z| taken inside the kernel (z_absmax=None: what the decode chain does) == the published scalar, bit for bit
        out2, t2 = ops.gemv_ln(zd, dev(w), dev(bias), dev(gn), dev(bn), eps, z_absmax=None, post=(dev(gp), dev(bp)), residual=resd,
                               want_t=True, gelu=gelu)
        assert torch.equal(out2, out) and torch.equal(t2, t)
    assert rel(out, out_ref.float().cpu()) < 2e-3 if dtype == torch.float16 else rel(out, out_ref.float().cpu()) < 1.5e-2
    assert abs(slot.item() - slot_ref.item()) <= 2e-2 * max(1.0, slot_ref.item())
    # oracle definition
    tf = (res.float() + O.sandwich_layernorm(z.float(), gp.float(), bp.float(), eps).to(dtype).float()).to(dtype).float() if post else z.float()
    xin = O.sandwich_layernorm(tf, gn.float(), bn.float(), eps).to(dtype).float()
    ref = O.linear(xin, w.float(), bias.float())
    if gelu:
        ref = O.gelu(ref.to(dtype).float())
    assert rel(out, ref) < TOL[dtype]


def test_attention_launch_order_independence(ops):
    """Every attention instantiation raises its own dynamic-LDS attribute at its first launch (attention.hip: attn_launch), so no
    result may depend on which form ran first: forward and backward of the four forms (dense without dropout, regenerating, stored
    keep bits, flexible: mask tensor and sparse training form) in both dtypes, in one order and then in the reverse order in the
    same process, bit-identical.  B = 1, H = 3 (fewer units than XCDs: idle workgroups), s = 192 (a full and a half query block:
    inactive waves); the sparse form at window 128, s = 256, 24 pivots + 2 windows = 280 slots."""
    from cogview_amd import functional as F_
    g = torch.Generator().manual_seed(192)
    drop = (0.1, 77, 5)
    s, w, times, n_piv = 192, 128, 2, 24
    data = {}
    for dtype in DTYPES:
        q, k, v, dout = [dev(rnd((1, s, 3, 64), dtype, g)) for _ in range(4)]
        mask = dev((torch.rand((1, s, s), generator=g) < 0.7).to(dtype))
        sq, sk, sv, sdout = [dev(rnd((1, 2 * w, 3, 64), dtype, g)) for _ in range(4)]
        pivot_idx = dev(torch.stack([torch.randperm(2 * w, generator=g)[:n_piv]]))
        tab, inv = F_.sparse_pivot_plan(pivot_idx, 2 * w, w, times)
        data[dtype] = (q, k, v, dout, mask, sq, sk, sv, sdout, tab, inv)

    def run(form, dtype):
        q, k, v, dout, mask, sq, sk, sv, sdout, tab, inv = data[dtype]
        if form == "dense":
            o, lse = ops.attention_fwd(q, k, v)
            return (o, lse) + tuple(ops.attention_bwd(dout, q, k, v, o, lse))
        if form == "regenerating":
            o, lse = ops.attention_fwd(q, k, v, dropout=drop)
            return (o, lse) + tuple(ops.attention_bwd(dout, q, k, v, o, lse, dropout=drop))
        if form == "stored bits":
            o, lse, bits = ops.attention_fwd(q, k, v, dropout=drop, keep_bits=True)
            # the keep words the forward pass wrote: query q's words of key blocks 0 .. q // 64 (those of blocks above its wave's
            # diagonal are never written and stay whatever the allocator handed out)
            words = bits.view(torch.int32).view(1, 3, (s + 63) // 64, 2, s)
            wrote = dev(torch.arange((s + 63) // 64).view(-1, 1, 1) <= (torch.arange(s) // 64).view(1, 1, -1)).expand_as(words)
            return (o, lse, words[wrote]) + tuple(ops.attention_bwd(dout, q, k, v, o, lse, dropout=drop, keep_bits=bits))
        if form == "mask tensor":
            o, lse = ops.attention_fwd(q, k, v, mask=mask)
            return (o, lse) + tuple(ops.attention_bwd(dout, q, k, v, o, lse, mask=mask))
        sp = (w, n_piv, math.log(2 * w // n_piv))
        o, lse = ops.attention_fwd(sq, sk, sv, kv_index=tab, sparse=sp, dropout=drop)
        return (o, lse) + tuple(ops.sparse_attention_bwd(sdout, sq, sk, sv, o, lse, tab, sp, inv, times, dropout=drop))

    order = [(f, d) for f in ("dense", "regenerating", "stored bits", "mask tensor", "sparse training") for d in DTYPES]
    first = {key: [t.clone() for t in run(*key)] for key in order}
    for key in reversed(order):
        again = run(*key)
        assert len(again) == len(first[key])
        for i, (a, b) in enumerate(zip(again, first[key])):
            assert torch.equal(a, b), (key, i)
