"""CPU: what the attention cell sweep (tests/attention_cells.py, run on the GPU by tests/test_attention_cells_gpu.py) rests on.
1. every row of the shape grid plans the form, the grids and the block counts its comment names (cogv_attention_plan plus the
   kernels' block arithmetic restated in Python); 2. the fp64 references agree with the oracle's and the keep-word decoder inverts
   the documented layout; 3. the checks check: an fp32 emulation of the kernels' arithmetic passes them on the whole grid with every
   ratio below 1, and each seeded mutant of it is rejected on the shape named for it; 4. the preconditions of the exact cells."""
import ctypes

import pytest
import torch

from cogview_amd import _lib
from oracle import cogview_oracle as O
from tests import attention_cells as AC

DTYPES = AC.DTYPES
IDS = [AC.DT_NAME[d] for d in DTYPES]


def plan(d, backward):
    out = (ctypes.c_int * 8)(*([-1] * 8))
    return _lib.lib().cogv_attention_plan(ctypes.byref(d), int(backward), out), list(out)


# ---------------------------------------------------------------------------------------------------------------- 1. the grid
@pytest.mark.parametrize("shape,want", AC.GRID, ids=[str(s) for s in AC.SHAPES])
def test_grid_row_reaches_what_it_names(shape, want):
    B, H, s_q, s_k, sep = shape
    grid_q, grid_k, sep_k, nkb, waves, stages = want
    S = AC.Staged(AC.problem("DENSE", shape, "randn", torch.float16), "cpu")
    assert plan(S.desc(), 0) == (_lib.OK, [AC.DENSE, 256, grid_q, 32768, 0, 0, B, sep_k])
    assert plan(S.desc(), 1) == (_lib.OK, [AC.DENSE, 256, grid_q, 35840, grid_k, 35840, B, sep_k])
    assert AC.geometry(s_q, s_k, sep) == (s_k - s_q, sep_k)
    units, nblk_q, nblk_k = B * H, (s_q + 127) // 128, (s_k + 127) // 128
    assert grid_q == 8 * ((units + 7) // 8) * nblk_q and grid_k == 8 * ((units + 7) // 8) * nblk_k
    fb = AC.fwd_blocks(s_q, s_k, sep_k)
    assert tuple(n for n, _ in fb) == nkb and tuple(len(w) for _, w in fb) == waves
    kb = AC.dkdv_blocks(s_q, s_k, sep_k)
    assert tuple(nqb - qb0 for qb0, nqb in kb) == stages
    # every wave's last key block is inside the workgroup's, and the heaviest workgroup reaches the last key
    assert all(max(w) <= 64 * n and (max(w) + 63) // 64 == n for n, w in fb) and max(max(w) for _, w in fb) == s_k


def test_grid_covers_the_paths_the_sweep_is_for():
    G = dict(AC.GRID)
    # a second and a third round per XCD: workgroups of units >= H B must return
    assert G[(3, 3, 129, 129, 0)][0] - 9 * 2 == 14 and G[(1, 17, 40, 40, 0)][0] - 17 == 7
    # both ring stages used an odd and an even number of times, forward / dQ and dK.dV
    assert {n % 2 for n in G[(1, 1, 257, 257, 0)][3]} == {0, 1} and {n % 2 for n in G[(1, 1, 130, 194, 70)][3]} == {0, 1}
    assert G[(1, 1, 257, 257, 0)][5] == (5, 3, 1)
    # tails: one key and one query alone in a tile / a wave
    assert 65 % 64 == 1 and AC.fwd_blocks(65, 65, 0)[0][1] == [32, 64, 65]
    # inactive waves: fewer than four in the only workgroup
    assert G[(1, 3, 64, 64, 0)][4] == (2,) and G[(1, 1, 1, 200, 0)][4] == (1,)
    # the prefix rule: one key past the first tile; across a workgroup of keys (its second key block starts at query 0)
    assert G[(1, 2, 96, 160, 5)][2] == 64 + 5 and G[(1, 1, 130, 194, 70)][2] == 134 > 128
    assert AC.dkdv_blocks(130, 194, 134)[1][0] == 0 and AC.dkdv_blocks(130, 194, 0)[1][0] == 1
    assert G[(1, 1, 100, 100, 200)][2] > 100
    # memory form: more key workgroups than query workgroups
    assert G[(1, 2, 33, 161, 0)][1] == 2 * G[(1, 2, 33, 161, 0)][0]
    # the mask tensors run where sep == 0; counts of the sweep
    assert len(AC.SHAPES) == 14 and len(AC.shapes_of("MASK_THREE")) == 10
    assert [AC.cells_of(f) for f in AC.FORMS] == [42, 42, 42, 30, 10, 10]


@pytest.mark.parametrize("form", tuple(AC.FORMS))
def test_forms_plan_their_instantiation(form):
    for shape in ((3, 3, 129, 129, 0), (1, 1, 1, 1, 0)):
        P = AC.problem(form, shape, "randn", torch.bfloat16)
        d = AC.Staged(P, "cpu").desc()
        for backward in (0, 1):
            rc, out = plan(d, backward)
            assert rc == _lib.OK and out[0] == P.plan_form == AC.FORMS[form][0], (form, shape, out)
            if AC.FORMS[form][3]:
                assert out[7] == shape[3]                                 # a mask tensor: every key is a candidate
        assert (d.mask_bs == 0) == (form != "MASK_RANDOM" and form != "MASK_THREE" or shape[0] == 1)


def test_factors_and_bookkeeping():
    assert all(1.0 <= f <= 2.0 for f in AC.FACTOR.values())
    assert set(AC.MUTANTS) and all(AC.MUTANTS[m][1] in AC.SHAPES for m in AC.MUTANTS)


# ---------------------------------------------------------------------------------------------------------------- 2. reference pins
@pytest.mark.parametrize("form,shape", [("DENSE", (3, 3, 129, 129, 0)), ("DENSE_DROP", (1, 2, 96, 160, 5)), ("DENSE", (1, 1, 100, 100, 200)),
                                        ("MASK_RANDOM", (2, 1, 65, 65, 0)), ("MASK_THREE", (1, 2, 33, 161, 0)), ("MASK_LTR", (1, 1, 257, 257, 0))])
def test_reference_is_the_oracles(form, shape):
    """the fp64 reference of the cells module against O.standard_attention in fp64, autograd for the gradients"""
    P = AC.problem(form, shape, "randn", torch.float16)
    ref, _ = AC.reference(P.q, P.k, P.v, P.do, AC.visibility(P), P.keep, P.p, P.dtype)
    q, k, v = [t.clone().requires_grad_(True) for t in (P.q, P.k, P.v)]
    mask = P.M.unsqueeze(1) if P.M is not None else O.build_mask(P.s_q, P.s_k, P.sep, torch.float64)
    # (the oracle's mask carries 1 / (1 - p) rounded to fp32; its keep decisions with the scale in fp64)
    drop = None if P.keep is None else (torch.from_numpy(O.attention_keep_mask(P.B, P.H, P.s_q, P.s_k, P.p, AC.SEED, AC.STREAM)) > 0).double() * \
        (65536.0 / (65536.0 - O._thr16(P.p)))
    out = O.standard_attention(q, k, v, mask, drop)
    out.backward(P.do)
    for name, a in (("o", out.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        assert float((ref[name] - a).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max())), name
    s = O.math.sqrt(64)
    scores = (P.q / s) @ P.k.transpose(-1, -2)
    scores = scores * mask - 10000.0 * (1.0 - mask)
    assert float((ref["lse"] - torch.logsumexp(scores, -1)).abs().max()) <= 1e-12 * 10000
    if form == "MASK_RANDOM":                                             # a fully masked row: uniform attention over ALL keys
        plain, _ = AC.reference(P.q, P.k, P.v, P.do, AC.visibility(P), None, 0.0, P.dtype)
        assert torch.allclose(plain["o"][:, :, -1], P.v.mean(2), rtol=0, atol=1e-9)


def _pack_slow(keep, s_q, s_k):
    """AttnArgs::keepbits restated word by word: word [(b H + head)][kb][fg][q], bit 31 - n <-> key 64 kb + 32 (n >> 4) +
    8 ((n & 15) >> 2) + 4 fg + (n & 3)"""
    B, H = keep.shape[:2]
    nkb = (s_k + 63) // 64
    words = torch.zeros(B * H * nkb * 2 * s_q, dtype=torch.int64)
    for b in range(B):
        for h in range(H):
            for kb in range(nkb):
                for fg in range(2):
                    for q in range(s_q):
                        w = 0
                        for n in range(32):
                            key = 64 * kb + 32 * (n >> 4) + 8 * ((n & 15) >> 2) + 4 * fg + (n & 3)
                            if key < s_k and bool(keep[b, h, q, key]):
                                w |= 1 << (31 - n)
                        words[(((b * H + h) * nkb + kb) * 2 + fg) * s_q + q] = w - (1 << 32) if w >= (1 << 31) else w
    return words.to(torch.int32)


def test_keep_word_decoder_round_trip():
    B, H, s_q, s_k = 1, 2, 5, 70
    keep = AC.keep_mask(B, H, s_q, s_k, 0.5)
    words = _pack_slow(keep, s_q, s_k)
    assert words.numel() == AC.keep_words_count(B, H, s_q, s_k) == _lib.lib().cogv_attention_keep_bits_bytes(B, H, s_q, s_k) // 4
    got = AC.decode_keep_words(words, B, H, s_q, s_k)
    assert torch.equal(got[..., :s_k], keep) and not bool(got[..., s_k:].any())
    # every bit of a word is one key of its block, each key once
    assert sorted(AC.KEY_OF_BIT.flatten().tolist()) == list(range(64))
    # the words the forward pass writes: key blocks that start below kend_w of the query's 32-row group
    w = AC.written_keep_slots(130, 194, 134)
    assert bool(w[0, :192].all()) and not bool(w[0, 192:].any()) and bool(w[128, :194].all()) and not bool(w[128, 194:].any())
    assert not bool(AC.written_keep_slots(65, 65, 0)[31, 64:].any()) and bool(AC.written_keep_slots(65, 65, 0)[64, 64])


# ---------------------------------------------------------------------------------------------------------------- 3. the checker checks
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", tuple(AC.FORMS))
def test_emulation_passes_every_check(form, dtype):
    fails, ran, refused, cells, worst = AC.sweep(AC.Emulated(), form, dtype)
    for name, r in sorted(worst.items()):
        print(f"RATIO emulation {form} {AC.DT_NAME[dtype]} {name}: worst err / bound = {r:.4f}")
    assert not fails, "\n".join(fails[:20])
    assert ran == cells == AC.cells_of(form) and refused == 0
    assert all(r < 1.0 for r in worst.values()), worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mutant", tuple(AC.MUTANTS))
def test_mutant_is_rejected(mutant, dtype):
    form, shape, kind = AC.MUTANTS[mutant]
    P = AC.problem(form, shape, kind, dtype)
    fails, _, rc = AC.run_cell(AC.Emulated(mutant), P)
    assert rc == _lib.OK and fails, mutant
    clean, _, _ = AC.run_cell(AC.Emulated(), P)
    assert not clean, clean
    print(f"{mutant} on {AC.cell_tag(form, shape, kind, dtype)}: " + "; ".join(fails[:3]))


# ---------------------------------------------------------------------------------------------------------------- 4. preconditions
@pytest.mark.parametrize("shape", AC.SHAPES, ids=[str(s) for s in AC.SHAPES])
def test_selector_preconditions(shape):
    B, H, s_q, s_k, sep = shape
    off, sep_k = AC.geometry(s_q, s_k, sep)
    for kind in ("selector", "decoy"):
        P = AC.problem("DENSE_DROP", shape, kind, torch.bfloat16)
        assert AC.min_hamming(P.k) >= 12, (shape, AC.min_hamming(P.k))
        vis = AC.ltr_visible(s_q, s_k, sep_k)
        assert bool(vis[torch.arange(s_q), P.sel].all())                  # every selected key is visible
        count = torch.zeros((B, H, s_k)).scatter_add_(2, P.sel, torch.ones((B, H, s_q)))
        assert float(count.max()) <= AC.MAX_SELECTORS
        assert float((P.v == 0).sum()) == 0 and float(P.v.abs().max()) <= 8 and float(P.do.min()) >= 1 and float(P.do.max()) <= 8
        sums = torch.zeros((B, H, s_k, 64), dtype=torch.float64).scatter_add_(2, P.sel.unsqueeze(-1).expand(B, H, s_q, 64), 2.0 * P.do)
        assert float(sums.max()) <= AC.EXACT_MAX[torch.bfloat16] and 2.0 * 8 <= AC.EXACT_MAX[torch.bfloat16]
        # the selected score is 128, every other visible key at least 48 lower
        S = AC.SCALE * (P.q @ P.k.transpose(-1, -2))
        if kind == "selector":
            top = torch.gather(S, 3, P.sel.unsqueeze(-1))
            assert bool((top == 128).all())
            others = S.masked_fill(~vis, -1e9).scatter(3, P.sel.unsqueeze(-1), -1e9)
            assert float(others.max()) <= 128 - 48
            assert bool((P.sel[..., 0] == off).all()) and bool((P.sel[..., -1] == s_q - 1 + off).all())
            if 0 < sep_k and off < min(sep_k, s_k) - 1 and s_q > 1:
                assert bool((P.sel == min(sep_k, s_k) - 1).any())          # a key only the prefix rule shows
        else:
            t = torch.arange(s_q) + off + 1
            aimed = (t < s_k) & (t >= sep_k)
            assert bool((P.aim[..., aimed] == t[aimed]).all()) and not bool(vis[torch.arange(s_q)[aimed], t[aimed]].any())
            if s_q > 1 and sep_k < s_k:
                assert bool(aimed.any())
        if s_q * B * H >= 16:                                             # at p = 0.5 both kept and dropped selectors occur
            hit = torch.gather(P.keep, 3, P.sel.unsqueeze(-1))
            assert bool(hit.any()) and not bool(hit.all())


def test_refusal_descriptors_are_refused_by_the_plan():
    """(g) on the CPU: the plan's code for every descriptor the GPU test hands to the launching entry points"""
    class PlanOnly:
        device = "cpu"

        def forward(self, S, d):
            return plan(d, 0)[0]

        def backward(self, S, d):
            return plan(d, 1)[0]
    fails, n = AC.refusal_sweep(PlanOnly(), torch.float16)
    assert not fails and n == len(AC.REFUSALS), fails


# ---------------------------------------------------------------------------------------------------------------- (f) sparse forms
@pytest.mark.parametrize("form,s", [("SPARSE", None), ("SPARSE_DROP", None), ("SPARSE", 640)])
def test_sparse_reference_is_the_oracles(form, s):
    """the slot-space reference, built from the table's semantics, against O.sparse_attention in fp64 (autograd for the gradients,
    the slot-space dK / dV folded as cogv_sparse_slot_reduce documents)"""
    P = AC.sparse_problem(form, torch.float16, s)
    w, n_piv, bias = P.sparse
    B, H, s = P.B, P.H, P.s_q
    G = s // w
    assert P.index.shape == (B, G, P.s_k) and P.s_k == n_piv + P.times * w
    d = AC.Staged(P, "cpu", kv_rows=s, planes=B * G).desc()
    assert plan(d, 0)[0] == _lib.OK and plan(d, 1)[1][0] == AC.FLEXIBLE and plan(d, 1)[1][6] == B * G
    ref, _ = AC._slots_reference(P)
    pam = O.sparse_rmask(s, w, P.times).double().expand(B, s, s).gather(-1, P.pivot_idx.unsqueeze(1).expand(B, s, n_piv))
    q, k, v = [t.clone().requires_grad_(True) for t in (P.q, P.kpool, P.vpool)]
    if P.keep is None:
        out = O.sparse_attention(q, k, v, P.pivot_idx, pam, w, P.times)
        out.backward(P.do)
        pairs = (("o", ref["o"].reshape(B, H, s, 64), out.detach()), ("dq", ref["dq"].reshape(B, H, s, 64), q.grad),
                 ("dk", AC.fold_slots(ref["dk"], P.pivot_idx, s, w, P.times), k.grad),
                 ("dv", AC.fold_slots(ref["dv"], P.pivot_idx, s, w, P.times), v.grad))
        for name, a, b in pairs:
            assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), name
    else:                                                                 # dropout: the adjoint identity <dO, O> == <dV, V> in slot space
        plain, _ = AC._slots_reference(AC.sparse_problem("SPARSE", torch.float16))
        assert float((plain["lse"] - ref["lse"]).abs().max()) == 0.0 and float((plain["o"] - ref["o"]).abs().max()) > 0.01
        dv = AC.fold_slots(ref["dv"], P.pivot_idx, s, w, P.times)
        lhs, rhs = float((P.do * ref["o"].reshape(B, H, s, 64)).sum()), float((dv * P.vpool).sum())
        assert abs(lhs - rhs) <= 1e-10 * abs(lhs)


@pytest.mark.parametrize("name", [c[0] for c in AC.GATHER_CELLS])
def test_gathered_reference_is_the_oracles(name):
    P = AC.gather_problem(name, torch.bfloat16)
    d = AC.Staged(P, "cpu", kv_rows=P.kpool.shape[2]).desc()
    assert plan(d, 0)[1][0] == AC.FLEXIBLE and plan(d, 1)[0] == _lib.ERR_UNSUPPORTED
    ref, _ = AC._slots_reference(P)
    flagged = P.index[0] < 0
    assert int(flagged.sum()) == (len(AC.GATHER_FLAGGED) if name == "sorted" else 0)
    if P.keep is None:                                                    # no flagged slot, no dropout: the oracle's gathered form
        out = O.sparse_attention_inference(P.q, P.kpool, P.vpool, P.index.to(torch.int64))
        assert float((ref["o"].squeeze(2) - out).abs().max()) <= 1e-12
    else:                                                                 # flagged slots carry no weight: the oracle without them
        idx = (P.index[0].to(torch.int64) & 0x7FFFFFFF)[~flagged].view(1, -1)
        plain, _ = AC.reference(P.q.unsqueeze(2), P.kpool[:, :, idx[0]].unsqueeze(2), P.vpool[:, :, idx[0]].unsqueeze(2), P.do.unsqueeze(2),
                                AC.ltr_visible(P.s_q, idx.shape[1], 0).double().view(1, 1, 1, P.s_q, -1), None, 0.0, P.dtype)
        out = O.sparse_attention_inference(P.q, P.kpool, P.vpool, idx)
        assert float((plain["o"].squeeze(2) - out).abs().max()) <= 1e-12
        undropped, _ = AC.reference(*[t.unsqueeze(2) for t in (P.q, P.kpool[:, :, P.index[0].to(torch.int64) & 0x7FFFFFFF],
                                                                P.vpool[:, :, P.index[0].to(torch.int64) & 0x7FFFFFFF], P.do)],
                                    (AC.ltr_visible(P.s_q, P.s_k, 0) & ~flagged.view(1, -1)).double().view(1, 1, 1, P.s_q, -1), None, 0.0, P.dtype)
        assert float((undropped["o"] - plain["o"]).abs().max()) <= 1e-12 and float((undropped["lse"] - ref["lse"]).abs().max()) == 0.0
