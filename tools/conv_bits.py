"""Bits of the tokenizer's forward convolutions, for comparing two builds of the library (a refactor of the kernels must not move
one): every cell of tests/vqvae_split_cases.py -- CELLS, EPILOGUE_CELLS x EPILOGUES, the fused-RGB cells, the two scales of
test_inputs_with_range -- in both precisions, on the library COGVIEW_HIP_LIB names (default: the tree's own).
    python tools/conv_bits.py dump OUT.pt          the outputs as int32 bit patterns
    python tools/conv_bits.py compare A.pt B.pt    one line per result; exit status 1 if any bit differs"""
import os, sys
import torch

if sys.argv[1] == "compare":
    a, b = torch.load(sys.argv[2]), torch.load(sys.argv[3])
    assert list(a) == list(b)
    bad = 0
    for k in a:
        same = a[k].shape == b[k].shape and torch.equal(a[k], b[k])
        bad += not same
        print(f"   {k}: {a[k].numel()} bit patterns {'equal' if same else 'DIFFER'} (first {a[k].view(-1)[0].item() & 0xffffffff:08x})")
    print(f"RESULT: {len(a)} results, {bad} differ" + ("" if bad else ": every bit identical"))
    sys.exit(1 if bad else 0)

assert sys.argv[1] == "dump"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cogview_amd import _lib
from tests import vqvae_split_cases as S

SCALE, SHIFT = (0.30379, 0.32279, 0.32800), (0.79093, 0.76271, 0.75340)
runs = [(f"cell {cell}", cell, {}, {}) for cell in S.CELLS]
runs += [(f"epilogue {cell} {e}", cell, {}, dict(epilogue=e)) for cell in S.EPILOGUE_CELLS for e in S.EPILOGUES]
runs += [(f"rgb {cell}", cell, {}, dict(rgb=(SCALE, SHIFT))) for cell in S.RGB_CELLS]
runs += [(f"range {S.RANGE_CELL} x {scale:g}", S.RANGE_CELL, dict(scale=scale), {}) for scale in (1e30, 1e-30)]
res = {}
for name, cell, make, run in runs:
    c = S.make_cell(*cell, **make)
    dev = S.device_cell(c)
    for precision in ("fp32", "bf16x3"):
        res[f"{name} | {precision}"] = S.run_cell(c, dev, precision, **run).contiguous().view(torch.int32).clone()
torch.cuda.synchronize()
torch.save(res, sys.argv[2])
print(f"{os.path.relpath(_lib.LIB_PATH)}: {len(res)} results saved to {sys.argv[2]}")
