"""CPU: the host side of the 4-bit (OCP MXFP4) decode weights -- the quantization rule on hand-made blocks, the torch
dequantizer, the new header entries, what weights="mxfp4" refuses, that the keyword reaches the decoder, the launch sequence of
the 4-bit step on recording stubs, and the 4-bit launch plans (cogv_gemv_w4_plan) with the proof that the GPU sweep of
tests/test_w4_gemv_gpu.py reaches every one of them."""
import os
import re
import types

import pytest
import torch

from cogview_amd import _lib
from cogview_amd.generation import DeviceFiller, GraphDecoder, SamplingDecoder, decoder, generate_on_device
from tests import gemv_cells as GC
from tests import w4_cases as W4
from tests.generation_cases import ToyIds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cogv_quantize_rows_mxfp4", "cogv_gemm_w4", "cogv_gemv_ln_w4", "cogv_gemv_attn_w4")


def _model(dtype=torch.float16, hidden=512, heads=8):
    from cogview_amd.model import GPT2Model
    torch.manual_seed(0)
    return GPT2Model(1, 64, hidden, heads, 0.0, 0.0, 0.0, 32, 32, False).to(dtype).eval()


def _args(**kw):
    return types.SimpleNamespace(**{**dict(temperature=1.0, top_k=1, top_p=0.0, is_sparse=0), **kw})


# ------------------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("dtype", W4.DTYPES, ids=GC.DT_NAME.get)
def test_the_rule_on_hand_made_blocks(dtype):
    """every tie (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5, 7 -> 0, 1, 1, 2, 2, 4, 4, 6), both signs, values just off the ties,
    saturation in (6, 8) * 2^e, a zero block (s = 127), a block at the exponent clamp (bf16: below 4 * 2^-126, s = 1)"""
    w, codes, scales = W4.crafted_rows(dtype)
    for quant in (W4.quantize, W4.quantize_float):
        q, s = quant(w)
        assert torch.equal(s.view(-1), scales), (quant.__name__, s.tolist())
        assert W4.same_codes(q, W4.pack(codes.view(1, -1))), (quant.__name__, (W4.unpack(q)[0] != codes).nonzero().flatten().tolist())
    ties = W4.dequantize(*W4.quantize(w))[0, :8]
    assert ties.tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0]
    assert int(W4.quantize(w)[1].min()) >= 1 and int(W4.quantize(w)[1].max()) <= 254


def test_nibble_order_and_scale_bytes():
    w = torch.zeros((1, 64), dtype=torch.float16)
    w[0, 0], w[0, 1], w[0, 2], w[0, 33] = 1.0, -0.5, 4.0, -3.0         # block 0: amax 4 -> e = 0; block 1: amax 3 -> e = -1
    q, s = W4.quantize(w)
    assert q[0, 0].item() == (0x2 | (0x9 << 4)) and q[0, 1].item() == 0x6 and q[0, 16].item() == (0xF << 4)
    assert s.tolist() == [[127, 126]]
    assert W4.dequantize(q, s)[0, [0, 1, 2, 33]].tolist() == [1.0, -0.5, 4.0, -3.0]


@pytest.mark.parametrize("dtype", W4.DTYPES, ids=GC.DT_NAME.get)
def test_integer_and_floating_point_forms_of_the_rule_agree(dtype):
    g = torch.Generator().manual_seed(4)
    w = (torch.randn((16, 512), generator=g) * torch.exp2(torch.randint(-20, 12, (16, 1), generator=g).float())).to(dtype)
    w[3, 32:64] = 0
    qa, sa = W4.quantize(w)
    qb, sb = W4.quantize_float(w)
    assert torch.equal(sa, sb) and W4.same_codes(qa, qb)
    # the error figure the issue quotes for Gaussian rows: relative weight error 0.114
    g2 = torch.randn((64, 2048), generator=g)
    dq = W4.dequantize(*W4.quantize(g2))
    err = ((dq - g2.double()).norm() / g2.double().norm()).item()
    assert 0.10 < err < 0.13, err


def test_torch_dequantizer_inverts_the_rule_on_representable_inputs():
    from cogview_amd import ops
    g = torch.Generator().manual_seed(5)
    nib = torch.randint(0, 16, (8, 256), generator=g)
    s = torch.randint(100, 140, (8, 8), generator=g).to(torch.uint8)
    nib[:, 31::32] = 6                                                    # a 4 * 2^e per block fixes the scale the quantizer finds
    q = W4.pack(nib)
    vals = ops.dequantize_rows_mxfp4(q, s)
    assert vals.dtype == torch.float32 and torch.equal(vals.double(), W4.dequantize(q, s))
    q2, s2 = W4.quantize(vals)
    assert torch.equal(s2, s) and W4.same_codes(q2, q)
    assert torch.equal(ops.dequantize_rows_mxfp4(q, s, torch.bfloat16).double(), vals.double())         # exact in bf16


# ------------------------------------------------------------------------------------------------------------ ABI
def test_new_header_entries_follow_the_abi_conventions():
    src = open(os.path.join(ROOT, "include", "cogview_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.lib()
    for name in NEW + ("cogv_gemv_w4_plan",):
        assert re.search(r"\bint %s\s*\(" % name, bare), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, bare, flags=re.S).group(1)
        assert res is _lib._i and len(args) == len(decl.split(",")), name
    for name in NEW:
        res, args = _lib.SIGNATURES[name]
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, bare, flags=re.S).group(1)
        assert args[-1] is _lib._vp and decl.split(",")[-1].strip() == "void* stream"
        head = src[:src.index("int %s(" % name)]
        comment = head[head.rindex("/*"):]
        assert re.search(r"[a-z_/]+\.py:\d+", comment), name
    body = re.search(r"typedef struct cogv_w4_weight \{(.*?)\} cogv_w4_weight;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _lib.W4Weight._fields_] == ["q", "ldq", "scale", "lds"]
    assert [f[0] for f in _lib.W8Weight._fields_] == ["q", "ldq", "scale"] and len(_lib.GemmDesc._fields_) == 27
    # argument errors come back as codes without a device
    assert lib.cogv_quantize_rows_mxfp4(0, None, 32, 1, 32, None, 16, None, 1, None) == 1
    assert lib.cogv_gemm_w4(None, None, None) == 1
    assert _lib.gemv_w4_plan(_lib.GEMV_PLAIN, _lib.F16, 1, 8, 512, ldq=250)[0] == _lib.ERR_ARG           # ldq % 16
    assert _lib.gemv_w4_plan(_lib.GEMV_PLAIN, _lib.F16, 1, 8, 512, lds=15)[0] == _lib.ERR_ARG            # lds < K / 32
    assert _lib.gemv_w4_plan(_lib.GEMV_PLAIN, _lib.F16, 1, 8, 512, ldq=272, lds=20)[0] == _lib.OK


# ------------------------------------------------------------------------------------------------------------ the decoder
def test_decoder_refuses_what_the_4bit_step_does_not_cover(monkeypatch):
    with pytest.raises(ValueError, match="weights="):
        GraphDecoder(_model(), weights="fp4")
    with pytest.raises(NotImplementedError, match="float32"):
        GraphDecoder(_model(torch.float32), weights="mxfp4")
    with pytest.raises(NotImplementedError, match="4-bit kernels"):
        GraphDecoder(_model(hidden=320, heads=5), weights="mxfp4")            # h % 512 != 0
    with pytest.raises(NotImplementedError, match="rows"):
        GraphDecoder(_model(), batch=9, weights="mxfp4")
    with pytest.raises(NotImplementedError, match="sparse"):
        generate_on_device(None, torch.tensor([1, 2, -1, -1]), _args(is_sparse=2), weights="mxfp4")
    with pytest.raises(NotImplementedError, match="sparse"):
        DeviceFiller(None, _args(is_sparse=2), weights="mxfp4")
    from cogview_amd.mpu import initialize
    monkeypatch.setattr(initialize, "mp_world_size_or_1", lambda: 2)
    with pytest.raises(NotImplementedError, match="model parallelism"):
        SamplingDecoder(_model(), weights="mxfp4")
    with pytest.raises(NotImplementedError, match="model parallelism"):
        generate_on_device(None, torch.tensor([1, 2, -1, -1]), _args(), weights="mxfp4")


def test_keyword_reaches_the_decoder(monkeypatch):
    seen = []

    class Stop(Exception):
        pass

    class Spy:
        def __init__(self, model, batch=1, capacity=1152, weights=None):
            seen.append((batch, weights))
            raise Stop

    monkeypatch.setattr(decoder, "SamplingDecoder", Spy)
    ids = ToyIds(32, 16)
    model = types.SimpleNamespace(word_embeddings=types.SimpleNamespace(weight=torch.zeros(56, 8)))
    seq = torch.tensor([40, ids["[BOI1]"], -3, -3, -3])
    with pytest.raises(Stop):
        generate_on_device(model, seq, _args(), tokenizer=ids, weights="mxfp4")
    f = DeviceFiller(model, _args(), weights="mxfp4")
    with pytest.raises(Stop):
        f(model, torch.tensor([40, ids["[BOI1]"], -1, 3, -1]), _args(), tokenizer=ids)
    assert seen == [(3, "mxfp4"), (1, "mxfp4")]


def test_default_decoder_holds_no_4bit_tensor():
    dec = GraphDecoder(_model(), batch=1, capacity=64)
    assert dec.w4 is None and dec.w8 is None and dec.wq is None


@pytest.mark.parametrize("fused", [True, False])
def test_4bit_step_launch_sequence_on_recording_stubs(monkeypatch, fused):
    """GraphDecoder(weights="mxfp4")._step on stubs (no GPU): every Linear product of the step is a 4-bit one reading the pair
    quantized from ITS weight, no 16-bit and no 8-bit product is called; fused: the chain's five launches per layer, else layer
    by layer with the Sandwich-LN launches -- the sequences tests/test_w8_cpu.py records for the 8-bit step."""
    from cogview_amd import functional as F_
    L_, V_, H_, NH_, B_ = 2, 64, 512, 8, 2
    from cogview_amd.model import GPT2Model
    m = GPT2Model(L_, V_, H_, NH_, 0.0, 0.0, 0.0, 32, 32, False).half().eval()
    calls, quantized = [], {}

    def _q(w):
        q, s = torch.zeros((w.shape[0], w.shape[1] // 2), dtype=torch.uint8), torch.full((w.shape[0], w.shape[1] // 32), 127, dtype=torch.uint8)
        quantized[id(q)] = w
        return q, s

    def _src(qs):
        return tuple(quantized[id(qs[0])].shape)

    def _never(*a, **k):
        raise AssertionError("a 16-bit or 8-bit product inside the 4-bit step")

    class Ops:
        quantize_rows_mxfp4 = staticmethod(_q)
        quantize_rows_e4m3 = gemm = gemv_ln = gemv_attn = gemm_w8 = gemv_ln_w8 = gemv_attn_w8 = staticmethod(_never)

        @staticmethod
        def scalar_slab(slab):
            import contextlib
            return contextlib.nullcontext()

        @staticmethod
        def gemv_ln_w4(z, qs, bias, gamma, beta, eps, z_absmax=None, post=None, residual=None, want_t=False, gelu=False, absmax=None):
            calls.append(("gemv_ln_w4", _src(qs), gelu))
            out = torch.zeros(z.shape[0], qs[0].shape[0], dtype=gamma.dtype)
            return out, (torch.zeros(z.shape, dtype=torch.float32) if (post is not None and want_t) else None)

        @staticmethod
        def gemm_w4(a, qs, bias=None, gelu=False, absmax=None):
            calls.append(("gemm_w4", _src(qs), gelu))
            return torch.zeros(a.shape[0], qs[0].shape[0], dtype=a.dtype)

        @staticmethod
        def gemv_attn_w4(parts, b, heads, cap, qs, dtype, bias=None, absmax=None):
            calls.append(("gemv_attn_w4", _src(qs), False))
            return torch.zeros(b, qs[0].shape[0], dtype=dtype)

        @staticmethod
        def attention_decode(qkv, cache, pos_index, heads, combine=True):
            calls.append(("attention_decode", combine))
            return torch.zeros(qkv.shape[0], 1, heads * 64, dtype=qkv.dtype)

        @staticmethod
        def sandwich_ln_fwd(x, gamma, beta, eps, absmax_in, residual=None, absmax_out=None, save_stats=True):
            calls.append(("ln",))
            return torch.zeros(x.shape, dtype=torch.float32 if residual is not None else gamma.dtype), None, None

        @staticmethod
        def new_absmax_slot(dev):
            return torch.zeros(1)

    monkeypatch.setattr(F_, "ops", Ops)
    monkeypatch.setattr(decoder, "ops", Ops)
    monkeypatch.setattr(F_, "_DECODE_FUSE_ENV", "1")
    dec = GraphDecoder(m, batch=B_, capacity=64, weights="mxfp4")
    assert dec.w8 is None and isinstance(dec.w4, F_.W4Weights) and dec.wq is dec.w4
    assert len(quantized) == 4 * L_ + 1 and _src(dec.w4.emb) == (V_, H_)
    assert len(dec.w4.tensors()) == 2 * (4 * L_ + 1) and all(t.dtype == torch.uint8 for t in dec.w4.tensors())
    dec.fused = fused
    tr = m.transformer
    h0 = torch.zeros(B_, 1, H_, dtype=torch.float32)
    h0._cogv_absmax = torch.ones(1)
    monkeypatch.setattr(type(tr), "embed", lambda self, tok, pos, emb: h0)
    logits = dec._step()
    assert logits.shape == (B_, 1, V_)
    shapes = [c[1] for c in calls if c[0].endswith("_w4")]
    assert shapes == [(3 * H_, H_), (H_, H_), (4 * H_, H_), (H_, 4 * H_)] * L_ + [(V_, H_)]
    assert [c[2] for c in calls if c[0].endswith("_w4")] == [False, False, True, False] * L_ + [False]
    names = [c[0] for c in calls]
    if fused:
        assert names == ["gemv_ln_w4", "attention_decode", "gemv_attn_w4", "gemv_ln_w4", "gemm_w4"] * L_ + ["gemv_ln_w4"]
        assert ("attention_decode", False) in calls
    else:
        assert names == ["ln", "gemm_w4", "attention_decode", "gemm_w4", "ln", "ln", "gemm_w4", "gemm_w4", "ln"] * L_ + ["ln", "gemm_w4"]


def test_decode_supported_asks_the_4bit_plan():
    from cogview_amd import functional as F_
    tr = _model().transformer
    assert F_.w4_decode_supported(tr, 1) is None and F_.w4_decode_supported(tr, 8) is None
    assert "8 rows" in F_.w4_decode_supported(tr, 9)
    assert "4-bit kernels" in F_.w4_decode_supported(_model(hidden=320, heads=5).transformer, 1)
    assert "8-bit kernels" in F_.w8_decode_supported(_model(hidden=320, heads=5).transformer, 1)


# ------------------------------------------------------------------------------------------------------------ the plans
V, M = 0, 1
UNTOUCHED = [-1] * _lib.GEMV_PLAN_INTS
# (kind, rows, K) at 136 columns -> (code, [generation, form, J | NWK, KCMAX | LMAX, guarded, MT, tiles, two halves, threads, grid, LDS])
SEEDS = [
    ("plain", 1, 1024, (0, [2, V, 16, 2, 0, 1, 1, 0, 256, 3, 2048])),
    ("attn", 1, 2560, (0, [2, V, 8, 5, 0, 1, 1, 0, 256, 5, 5120])),
    ("ln", 1, 2560, (0, [2, V, 4, 5, 0, 1, 1, 0, 256, 9, 5120])),
    ("ln", 1, 1024, (0, [2, V, 16, 2, 0, 1, 1, 0, 256, 3, 2048])),
    ("ln", 1, 1536, (0, [2, V, 2, 8, 1, 1, 1, 0, 256, 17, 3072])),
    ("plain", 1, 4096, (0, [2, V, 8, 8, 0, 1, 1, 0, 256, 5, 8192])),
    ("plain", 1, 10240, (0, [2, V, 4, 20, 0, 1, 1, 0, 256, 9, 20480])),
    ("plain", 1, 5632, (0, [2, V, 4, 20, 1, 1, 1, 0, 256, 9, 11264])),
    ("attn", 1, 4096, (0, [2, V, 4, 20, 1, 1, 1, 0, 256, 9, 8192])),
    ("plain", 2, 1024, (0, [2, M, 2, 4, 0, 2, 1, 0, 128, 9, 2 * 1032 * 2])),
    ("ln", 2, 1024, (0, [2, M, 2, 4, 0, 2, 2, 0, 256, 5, 2 * 1032 * 2])),
    ("ln", 8, 2560, (0, [2, M, 2, 10, 0, 8, 4, 0, 512, 3, 8 * 2568 * 2])),
    ("attn", 3, 2560, (0, [2, M, 2, 10, 0, 4, 1, 0, 128, 9, 4 * 2568 * 2])),
    ("plain", 4, 4096, (0, [2, M, 2, 16, 0, 4, 1, 0, 128, 9, 4 * 4104 * 2])),
    ("plain", 8, 4096, (0, [2, M, 2, 16, 0, 8, 1, 1, 128, 9, 8 * 2056 * 2])),
    ("plain", 2, 10240, (0, [2, M, 4, 20, 0, 2, 1, 0, 256, 9, 2 * 10248 * 2])),
    ("plain", 8, 10240, (0, [2, M, 4, 20, 0, 8, 1, 1, 256, 9, 8 * 5128 * 2])),
    ("plain", 2, 1536, (0, [2, M, 2, 20, 1, 2, 1, 0, 128, 9, 2 * 1544 * 2])),
    ("ln", 4, 3072, (0, [2, M, 2, 20, 1, 4, 4, 0, 512, 3, 4 * 3080 * 2])),
    ("ln", 2, 4096, (0, [2, M, 2, 20, 1, 2, 2, 0, 256, 5, 2 * 4104 * 2])),
    ("attn", 2, 4096, (0, [2, M, 2, 20, 1, 2, 1, 0, 128, 9, 2 * 4104 * 2])),
    ("plain", 5, 5120, (3, UNTOUCHED)),                                   # 8 x 5128 x 2 bytes of x rows: above the guarded classes' LDS
    ("plain", 4, 5120, (0, [2, M, 2, 20, 1, 4, 1, 0, 128, 9, 4 * 5128 * 2])),
    ("plain", 2, 5632, (3, UNTOUCHED)),
    ("ln", 8, 4096, (3, UNTOUCHED)),
    ("ln", 1, 4608, (3, UNTOUCHED)),
    ("plain", 1, 10752, (3, UNTOUCHED)),
]


@pytest.mark.parametrize("kind,rows,K,want", SEEDS)
def test_plan_table_as_literals(kind, rows, K, want):
    for dtype in W4.DTYPES:
        assert W4.plan(kind, dtype, rows, 136, K) == want, (kind, rows, K, dtype)


def test_the_4bit_plans_leave_the_other_formats_answers_alone():
    """the class ids of the 16-bit and the 8-bit rows did not move: the seeds of tests/test_gemv_plan.py, asked again here"""
    assert _lib.gemv_plan(_lib.GEMV_PLAIN, _lib.F16, 1, 136, 2560) == (0, [2, V, 4, 5, 0, 1, 1, 0, 256, 9, 5120])
    assert _lib.gemv_plan(_lib.GEMV_PLAIN, _lib.F16, 1, 136, 1024, w8=True) == (0, [2, V, 16, 2, 0, 1, 1, 0, 256, 3, 2048])
    assert _lib.gemv_plan(_lib.GEMV_LN, _lib.F16, 2, 136, 1024, w8=True) == (0, [2, M, 2, 8, 0, 2, 2, 0, 256, 5, 2 * 1032 * 2])


@pytest.mark.parametrize("kind", W4.KINDS)
def test_the_gpu_sweep_grid_reaches_every_4bit_plan(kind):
    """Every distinct plan the 4-bit list gives -- asked for every row count 1 .. 8 and every multiple of 512 up to 10240 -- is
    the plan of a point of tests/w4_cases.py's grid, in both dtypes; and where the list refuses, it refuses a grid point too."""
    for dtype in W4.DTYPES:
        want, refuses = set(), False
        for K in range(512, 10240 + 512, 512):
            for rows in range(1, 9):
                rc, out = W4.plan(kind, dtype, rows, 136, K, nsplit=32 if kind == "attn" else 1)
                if rc == _lib.OK:
                    assert out[0] == 2 and out[5] == {1: 1, 2: 2, 3: 4, 4: 4}.get(rows, 8)
                    want.add(GC.plan_id(out))
                else:
                    assert rc == _lib.ERR_UNSUPPORTED
                    refuses = True
        reached, grid_refuses = set(), False
        for K in W4.ks(kind):
            for rows in W4.MS:
                rc, out = W4.plan(kind, dtype, rows, 136, K, nsplit=32 if kind == "attn" else 1)
                if rc == _lib.OK:
                    reached.add(GC.plan_id(out))
                else:
                    grid_refuses = True
        assert len(want) >= 10 and not want - reached, (kind, dtype, sorted(want - reached))
        assert grid_refuses == refuses
    # the grid's column counts differ from every columns-per-workgroup choice of the list: 16, 32, 64, 128
    assert all(n % c for n in (40, 136) for c in (16, 32, 64, 128))
