"""CPU: the host side of on-device generation (generation.generate_on_device): the planning of context, run, beam count and
drawable range by filling_sequence's marker rule, its refusals, and the ctypes layout of cogv_sample_desc."""
import os
import re
import types

import pytest
import torch

from cogview_amd import _lib
from cogview_amd.generation import IdSpace, add_interlacing_beam_marks, generate_on_device, plan_device_generation
from tests.generation_cases import ToyIds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(seq, ids, vocab):
    return plan_device_generation(list(seq), ids, vocab)


@pytest.mark.parametrize("space", ["released", "toy"])
def test_plan_after_each_marker(space):
    ids = IdSpace() if space == "released" else ToyIds(8192, 500)
    n_img, n_txt = ids.img_tokenizer.num_tokens, ids.txt_tokenizer.num_tokens
    vocab = 58240 if space == "released" else 8704
    text = [n_img + 5, n_img + 17, n_img + 3]
    for boi in ("[BOI1]", "[BOI2]"):
        seq = text + [ids["[BASE]"], ids[boi]] + [-1] * 1024
        add_interlacing_beam_marks(seq, nb=8, period=3000)
        p = _plan(seq, ids, vocab)
        assert (p["context"], p["run"], p["nb"], p["allow"]) == (5, 1024, 8, (0, n_img)), p
        assert p["capacity"] >= len(seq) and p["capacity"] % 64 == 0 and p["offset"] == 100000
    # after an image: text pieces only
    p = _plan(text + [ids["[BOI1]"], 7, 9, ids["[EOI1]"]] + [-1] * 6, ids, vocab)
    assert (p["context"], p["run"], p["nb"], p["allow"]) == (7, 6, 1, (n_img, n_img + n_txt))
    # no marker at all: filling_sequence's initial slices forbid the image codes only
    p = _plan(text + [-2] * 4, ids, vocab)
    assert (p["nb"], p["allow"]) == (2, (n_img, vocab))
    # [ROI2] in the context: the positions after it restart (filling_sequence's offset)
    p = _plan(text + [ids["[ROI2]"], ids["[BOI2]"]] + [-1] * 3, ids, vocab)
    assert p["offset"] == 3 and p["allow"] == (0, n_img)


def test_plan_refusals():
    ids = ToyIds(8192, 500)
    ctx = [8300, ids["[BASE]"], ids["[BOI1]"]]
    with pytest.raises(NotImplementedError, match="filling_sequence"):
        _plan(ctx + [-1] * 4 + [ids["[EOI1]"]], ids, 8704)          # a given id after the run
    seq = ctx + [-1] * 10
    add_interlacing_beam_marks(seq, nb=4, period=4)                  # 4, 3, 4 beams
    with pytest.raises(NotImplementedError, match="filling_sequence"):
        _plan(seq, ids, 8704)
    with pytest.raises(NotImplementedError, match="4096"):
        _plan(ctx + [-1] * 4200, ids, 8704)
    with pytest.raises(ValueError):
        _plan(ctx, ids, 8704)                                         # nothing to generate
    with pytest.raises(ValueError):
        _plan([-1, -1], ids, 8704)                                    # no context


def test_generate_on_device_refuses_sparse_before_touching_the_model():
    args = types.SimpleNamespace(temperature=1.0, top_k=1, top_p=0.0, is_sparse=2)
    with pytest.raises(NotImplementedError, match="filling_sequence"):
        generate_on_device(None, torch.tensor([1, 2, -1]), args)


def test_sample_desc_field_order_matches_header():
    src = open(os.path.join(ROOT, "include", "cogview_hip.h")).read()
    body = re.search(r"typedef struct cogv_sample_desc \{(.*?)\} cogv_sample_desc;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            for part in decl.split(","):
                names.append(re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part.split("[")[0])[-1])
    assert names == [f[0] for f in _lib.SampleDesc._fields_]
    assert "cogv_sample_logits" in _lib.SIGNATURES
