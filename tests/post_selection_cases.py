"""Shared by the post-selection tests (CPU emulation and GPU): the golden's two scoring rows (tests/golden/generate_samples.npz
`sel_seq`, `sel_scores`: the reference's own inverse_prompt_score on the reference's fp32 model) and the same rows moved
into the layout text-to-image generation returns."""
import types

import torch

from tests.generation_cases import ToyIds, load_golden

SCORE_ATOL = 5e-3            # the bar tests/generation_cases.py run_generation_golden_case holds the host path to
IMAGE_TOKENS = 1024          # the reference's scoring rows: [BASE] [BOI1] 1024 codes [EOI1] [ROI1] text...


def golden_case(golden_dir):
    z, c = load_golden(golden_dir)
    ids = ToyIds(c["img_tokens"], c["txt_tokens"])
    args = types.SimpleNamespace(temperature=1.0, top_k=1, top_p=0.0, is_sparse=0)
    return z, c, ids, args


def generated_rows(z, ids, dev):
    """sel_seq as generate_on_device / filling_sequence would have returned it: [ROI1] text [BASE] [BOI1] codes."""
    sel = torch.from_numpy(z["sel_seq"]).to(dev)
    assert sel.shape[1] > IMAGE_TOKENS + 4 and bool((sel[:, IMAGE_TOKENS + 3] == ids["[ROI1]"]).all())
    roi1 = sel[:, IMAGE_TOKENS + 3: IMAGE_TOKENS + 4]
    return torch.cat((roi1, sel[:, IMAGE_TOKENS + 4:], sel[:, :2], sel[:, 2:2 + IMAGE_TOKENS]), dim=1)
