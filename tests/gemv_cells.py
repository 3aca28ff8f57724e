"""Shared body of the skinny-M (M <= 8) cell sweep: the grid every launch plan of csrc/gemv_plan.h must have a point in
(tests/test_gemv_plan.py proves that on the CPU), the operands and fp64 references of the exact-integer product, and the
element-wise bound of the `randn` product.  tests/test_gemv_cells_gpu.py runs it; so does the child process that test starts
under COGV_GEMV2=0 (python -m tests.gemv_cells).

Exact-integer product: x, W in {-1, 0, 1} and an integer bias.  Every partial sum is an integer far below 2^24, so an fp32 sum
in ANY association is exact and the result, an integer the output type holds, equals the fp64 one to the bit -- in every class,
in the first-generation kernels and in the two-halves kernel.  One dropped or doubled contraction slot changes an integer."""
import sys

import torch

from cogview_amd import _lib

FORMATS = (False, True)                                          # 16-bit weights | E4M3 bytes + one fp32 scale per row
KINDS = ("plain", "attn", "ln")
DTYPES = (torch.float16, torch.bfloat16)
MS = (1, 2, 3, 4, 5, 8)
NS = (8, 40, 136)
KS = (512, 1024, 1536, 2560, 3072, 3584, 4096, 5120, 5632, 9728, 10240)
LN_MAX_K = 4096
M_MAX, N_MAX = max(MS), max(NS)
KIND_CODE = {"plain": _lib.GEMV_PLAIN, "attn": _lib.GEMV_ATTN, "ln": _lib.GEMV_LN}
DT_CODE = {torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}
DT_NAME = {torch.float16: "fp16", torch.bfloat16: "bf16"}
CAPS = (128, 4096)                                               # attn kind: 1 and 32 key splits
LN_STREAM32_KS = (512, 1024, 2560, 3072, 4096)                   # one K per class of the LayerNorm kind, at every row bucket
EPS = 1e-5

# integers the output type holds exactly: 11 / 8 significand bits
EXACT_MAX = {torch.float16: 2048, torch.bfloat16: 256}
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}       # one rounding of the output
# x is non-zero with probability 1/2 and W with 1/8: K / 16 non-zero products of +-1, a sum of standard deviation 25 at
# K = 10240; |bias| <= 4.  The 8 x 136 sums of a K stay below 6 sigma + 4 = 156 < 256 (asserted per K before any launch).
X_DENSITY, W_DENSITY, BIAS_MAX = 0.5, 0.125, 4
# factor on the element-wise bound per form (1: the bound as derived; see DESIGN 4.5.1 for the measured ratios)
BOUND_FACTOR = {"V": 1.0, "M": 1.0, "M-k2": 1.0, "gen1": 1.0}


def ks(kind):
    return tuple(K for K in KS if kind != "ln" or K <= LN_MAX_K)


def plan(kind, w8, dtype, M, N, K, nsplit=1):
    """(code, the 11 integers of cogv_gemv_plan) of a contiguous product"""
    return _lib.gemv_plan(KIND_CODE[kind], DT_CODE[dtype], M, N, K, w8=w8, nsplit=nsplit)


def plan_id(out):
    """what identifies a plan besides its grid: (generation, form, J | NWK, KCMAX | LMAX, guarded, tiles, two halves, MT)"""
    return (out[0], out[1], out[2], out[3], out[4], out[6], out[7], out[5])


def form_name(out):
    return "gen1" if out[0] == 1 else ("V", "M")[out[1]] + ("-k2" if out[7] else "")


def ternary(shape, density, gen):
    """fp64 values in {-1, 0, 1}, non-zero with probability `density`"""
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    return sign * (torch.rand(shape, generator=gen) < density).double()


def exact_operands(K, dtype):
    """x [8, K], W [136, K], bias [136], ref [8, 136] = x W^T + bias in fp64; smaller cells take leading rows"""
    g = torch.Generator().manual_seed(K)
    x, w = ternary((M_MAX, K), X_DENSITY, g), ternary((N_MAX, K), W_DENSITY, g)
    bias = torch.randint(-BIAS_MAX, BIAS_MAX + 1, (N_MAX,), generator=g).double()
    dot = x @ w.t()
    ref = dot + bias
    assert float(ref.abs().max()) <= EXACT_MAX[dtype], (K, float(ref.abs().max()))
    return x, w, bias, dot, ref


def e4m3_bytes(w):
    """{-1, 0, 1} -> the E4M3 bytes 0xB8, 0x00, 0x38"""
    return torch.where(w > 0, 0x38, torch.where(w < 0, 0xB8, 0)).to(torch.uint8)


def partials(x, nsplit):
    """The decode attention's partials [row][head][split][66] fp32 (m in the log2 domain, l, o[64]) whose combination is x
    [rows, heads * 64] exactly: equal m = 0 everywhere, and head h keeps (l = 1, o = x) in split h % nsplit, (0, 0) elsewhere."""
    rows, heads = x.shape[0], x.shape[1] // 64
    p = torch.zeros((rows, heads, nsplit, 66), dtype=torch.float32, device=x.device)
    h = torch.arange(heads, device=x.device)
    p[:, h, h % nsplit, 1] = 1.0
    p[:, h, h % nsplit, 2:] = x.float().view(rows, heads, 64)
    return p


def bound(ref, absdot, bias, K, dtype, x_rounded=False):
    """|got - ref| <= u |ref| + 2 K 2^-24 (|x| |W|^T |scale| + |bias|) + 2^-24: one rounding of the output, twice the textbook
    bound of an fp32 sum of K products in any order; x_rounded (attn kind: the combined x is rounded to the storage type inside
    the kernel) adds u |x| |W|^T."""
    b = U[dtype] * ref.abs() + 2.0 * K * 2.0 ** -24 * (absdot + bias.abs()) + 2.0 ** -24
    return b + U[dtype] * absdot if x_rounded else b


class Product:
    """One (kind, format, dtype, K): the device operands of the largest cell, launched at any (M, N) by leading rows."""

    def __init__(self, ops, kind, w8, dtype, K, x, w=None, bias=None, qs=None, z=None):
        self.ops, self.kind, self.w8, self.dtype, self.K = ops, kind, w8, dtype, K
        dev = "cuda"
        self.bias = None if bias is None else bias.to(dtype).to(dev)
        if w8:
            self.q, self.scale = (t.to(dev) for t in qs)
        else:
            self.w = w.to(dtype).to(dev)
        if kind == "plain":
            self.x = x.to(dtype).to(dev)
        elif kind == "attn":
            self.parts = {cap: partials(x.to(dev), (cap + 127) // 128) for cap in CAPS}
        else:
            # gamma = 0, beta = x: x_in is beta in every row, whatever z holds (z random: its variance must not vanish)
            self.z = z.to(dtype).to(dev)
            self.zero, self.zeros = torch.zeros(K, dtype=dtype, device=dev), torch.zeros((M_MAX, K), dtype=dtype, device=dev)
            self.beta = x[0].to(dtype).to(dev)

    def weight(self, N, scale=None):
        return (self.q[:N], (self.scale if scale is None else scale)[:N]) if self.w8 else self.w[:N]

    def __call__(self, M, N, bias=True, gelu=False, cap=128, post=False, scale=None):
        ops, b = self.ops, (self.bias[:N] if bias else None)
        w = self.weight(N, scale)
        if self.kind == "plain":
            return ops.gemm_w8(self.x[:M], w, bias=b, gelu=gelu) if self.w8 else ops.gemm(self.x[:M], w, bias=b, gelu=gelu)
        if self.kind == "attn":
            heads = self.K // 64
            if self.w8:
                return ops.gemv_attn_w8(self.parts[cap][:M], M, heads, cap, w, self.dtype, bias=b)
            return ops.gemv_attn(self.parts[cap][:M], M, heads, cap, w, bias=b)
        fn = ops.gemv_ln_w8 if self.w8 else ops.gemv_ln
        kw = dict(post=(self.zero, self.beta), residual=self.zeros[:M], want_t=True) if post else {}
        out, t = fn(self.z[:M], w, b, self.zero, self.beta, EPS, gelu=gelu, **kw)
        if post and not torch.equal(t, self.beta.expand(M, self.K)):
            return None
        return out


def exact_sweep(ops, kind, w8, dtype, ms=MS, ns=NS):
    """Checks (a) and (d) on every cell of the grid: -> (failures: one line each, launched cells, refused cells)"""
    fails, ran, refused = [], 0, 0
    tag = f"{kind} {'e4m3' if w8 else 'w16'} {DT_NAME[dtype]}"
    for K in ks(kind):
        x, w, bias, dot, ref = exact_operands(K, dtype)
        g = torch.Generator().manual_seed(K + 1)
        prod = Product(ops, kind, w8, dtype, K, x, w, bias, qs=(e4m3_bytes(w), torch.ones(N_MAX)), z=torch.randn((M_MAX, K), generator=g))
        if kind == "ln":                                      # every row of x_in is x[0]
            dot = dot[:1].expand(M_MAX, N_MAX)
            ref = dot + bias
        ref_d, dot_d = ref.to(dtype).cuda(), dot.cuda()
        assert torch.equal(ref_d.double().cpu(), ref)
        # second pass of the 8-bit format: a power of two per row, no bias (an integer times 2^e is held exactly)
        pow2 = torch.exp2(torch.randint(-3, 4, (N_MAX,), generator=g).float()).cuda()
        scaled_d = (dot_d * pow2.double()).to(dtype)
        for M in ms:
            for N in ns:
                rc, out = plan(kind, w8, dtype, M, N, K, nsplit=32 if kind == "attn" else 1)
                where = f"{tag} M={M} N={N} K={K}"
                if rc != _lib.OK:
                    refused += 1
                    try:
                        prod(M, N)
                        fails.append(f"{where}: the plan refuses ({rc}) but the call launched")
                    except _lib.CogviewHipError:
                        pass
                    continue
                ran += 1
                where += f" [{form_name(out)}]"
                variants = [dict(cap=cap) for cap in CAPS] if kind == "attn" else [dict(), dict(post=True)] if kind == "ln" else [dict()]
                for kw in variants:
                    got = prod(M, N, **kw)
                    if got is None:
                        fails.append(f"{where} {kw}: t is not beta_post")
                    elif got.shape != (M, N) or got.dtype != dtype or not torch.equal(got, ref_d[:M, :N]):
                        fails.append(f"{where} {kw}: {int((got != ref_d[:M, :N]).sum())} wrong elements")
                    elif not torch.equal(prod(M, N, **kw), got):
                        fails.append(f"{where} {kw}: the second call gives other bits")
                if w8:
                    got = prod(M, N, bias=False, scale=pow2)
                    if not torch.equal(got, scaled_d[:M, :N]):
                        fails.append(f"{where} row scales 2^e: {int((got != scaled_d[:M, :N]).sum())} wrong elements")
    return fails, ran, refused


def main():
    """the 16-bit exact sweep of all three kinds, one line per failure (the child process of the COGV_GEMV2=0 test)"""
    from cogview_amd import ops
    total = 0
    for kind in KINDS:
        for dtype in DTYPES:
            fails, ran, _ = exact_sweep(ops, kind, False, dtype)
            total += ran
            for line in fails:
                print("FAIL " + line)
            gens = {plan(kind, False, dtype, M, 136, K)[1][0] for K in ks(kind) for M in MS}
            print(f"generations {kind} {DT_NAME[dtype]}: {sorted(gens)}")
    print(f"cells {total}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
