"""GPU: post-selection on the device (generation.inverse_prompt_score_on_device, post_selection_rows, rerank_generated) on the
toy golden model, held to the scores the REFERENCE's inverse_prompt_score produced on the reference's own fp32 model
(tests/golden/generate_samples.npz `sel_seq` / `sel_scores`) at the bar the host path is held to (5e-3).  The device form is
NOT bit-equal to the host path or to its own chunked runs -- the logits product runs at another M and may split differently --
so those differences are printed, not asserted."""
import types

import numpy as np
import pytest
import torch

from tests.generation_cases import build_model
from tests.post_selection_cases import IMAGE_TOKENS, SCORE_ATOL, generated_rows, golden_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(golden_dir):
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    z, c, ids, args = golden_case(golden_dir)
    models = {kv: build_model(z, c, "cuda", kv) for kv in (False, True)}
    return types.SimpleNamespace(z=z, ids=ids, args=args, models=models, sel=torch.from_numpy(z["sel_seq"]).cuda(),
                                 rows=generated_rows(z, ids, "cuda"))


@pytest.mark.parametrize("kv_cache", [False, True])
def test_golden_scores(case, kv_cache):
    from cogview_amd.generation import inverse_prompt_score, inverse_prompt_score_on_device
    model, want = case.models[kv_cache], case.z["sel_scores"]
    whole = inverse_prompt_score_on_device(model, case.sel, case.args, tokenizer=case.ids)
    one = inverse_prompt_score_on_device(model, case.sel, case.args, tokenizer=case.ids, max_rows=1)
    host = inverse_prompt_score(model, case.sel, case.args, tokenizer=case.ids)
    for name, got in (("all rows", whole), ("max_rows = 1", one)):
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (2,)
        print(f"kv_cache={kv_cache} {name}: {got.tolist()}  golden {want.tolist()}  |diff| {np.abs(got.cpu().numpy() - want).max():.2e}")
    print(f"kv_cache={kv_cache}: device - host {(whole - host).abs().max().item():.2e}, whole - one row per forward "
          f"{(whole - one).abs().max().item():.2e}")
    for got in (whole, one):
        assert np.allclose(got.cpu().numpy(), want, rtol=0, atol=SCORE_ATOL), (got.tolist(), want.tolist())


def test_rows_are_rebuilt_exactly(case):
    from cogview_amd.generation import post_selection_rows
    out = post_selection_rows(case.rows, case.ids, IMAGE_TOKENS)
    assert out.is_cuda and torch.equal(out, case.sel)


def test_ranking(case):
    from cogview_amd.generation import rerank_generated
    want = case.z["sel_scores"]
    assert want[1] > want[0]
    best, scores, order = rerank_generated(case.models[True], case.rows, case.args, tokenizer=case.ids)
    assert best.is_cuda and scores.is_cuda and order.is_cuda
    assert order.tolist() == [1, 0] and torch.equal(best, case.rows[[1, 0]])
    assert np.allclose(scores.cpu().numpy(), want[[1, 0]], rtol=0, atol=SCORE_ATOL)
    best, scores, order = rerank_generated(case.models[True], case.rows, case.args, tokenizer=case.ids, keep=1)
    assert order.tolist() == [1] and torch.equal(best, case.rows[1:2]) and tuple(scores.shape) == (1,)


def test_refusals(case):
    from cogview_amd.generation import inverse_prompt_score_on_device
    model = case.models[False]
    with pytest.raises(NotImplementedError, match="inverse_prompt_score"):
        inverse_prompt_score_on_device(model, case.sel, types.SimpleNamespace(is_sparse=2), tokenizer=case.ids)
    bad = case.sel.clone()
    bad[1, 2 + IMAGE_TOKENS + 1] = case.ids["[EOI1]"]               # [ROI1] missing in the second row only
    with pytest.raises(ValueError):
        inverse_prompt_score_on_device(model, bad, case.args, tokenizer=case.ids)
    three = torch.cat((case.sel, case.sel[:1]), dim=0)
    with pytest.raises(ValueError):
        inverse_prompt_score_on_device(model, three, case.args, tokenizer=case.ids, max_rows=2)    # 3 >= 2 and 3 % 2 != 0
