"""Score-range tests of the decode and merge kernels — the decode-side counterpart of test_deferred_rescale_of_the_pipelined_kernel
(tests/test_gpu_attention.py), against fp64 with the project's `_check` (both bounds).  Forms: one-token (one and two head blocks), multi-token
(R = 16, 32, 64), windowed; launch plans: device-planned stream (default and forced grids) and the uniform grid split, asserted per case.
  late       a spike (score 110 above the rest) in the last tile of the last piece: the running maximum jumps late, every other piece's merge
             weight underflows to exactly 0
  early      a spike in the first tile of the first piece: the maximum only decreases afterwards
  one_piece  a spike in the middle, under num_splits in {0, -2, -50}
  empty      no visible key in a piece (partial LSE -inf) merged with live ones: one-tile pieces of a windowed multi-token call whose first tile
             holds a key for row 0 only, entries with dead rows, a windowed one-token call cut into more shares than it has visible tiles
  scale      softmax_scale in {1.0, 0.02, 1.7 D^-0.5}, the LSE against the oracle's
  v3e4       value rows of magnitude 3e4 in fp16: the output is near the top of the range and finite
The inputs and their scaling are written down in tests/census.py; tests/test_census_model.py asserts for every set that the oracle's own f32
math stays within half the tolerance of its f64 math."""
import pytest
import torch

from tests import census as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = C.numerics_cases()
_refs = {}


def _inputs_and_refs(c):
    key = C.inputs_key(c)
    if key not in _refs:
        _refs.clear()                  # (cases that share inputs are neighbours in the table)
        q, kc, vc = C.numerics_inputs(c)
        r64, l64 = C.reference(c, q, kc, vc, "f64", True)
        _refs[key] = (q, kc, vc, r64, l64, C.reference(c, q, kc, vc, "f32"))
    return _refs[key]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_decode_score_range(case):
    q, kc, vc, ref64, lse64, ref32 = _inputs_and_refs(case)
    out, lse, d = C.launch(case, q, kc, vc, DEV)
    what = "%s %s" % (case["name"], d)
    assert bool(torch.isfinite(out).all()), what
    if case["kind"] != "plain" or case["splits"] < 0 or case["path"] == 2:
        assert d["merge_launch"] == 1, what          # every spike case is about the merge of pieces
    C.check(out, ref64, ref32, C.DT[case["dt"]], what)
    C.check_lse(lse, lse64, what + " lse")
    if case["kind"] == "v3e4":
        assert float(out.float().abs().max()) > 2.5e4, what
