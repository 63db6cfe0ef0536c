"""What the two codecs compute from their packed weights, against the record of the build before the weight layouts were described once
(csrc/common.h `PackKind`): tests/golden/codec_pack_parent.npz (tools/make_codec_pack_golden.py, which states the cases).

tests/test_gpu_pack.py holds each layout equal to its restatement; this holds the WIRING equal -- which parameter goes where in which
layout, as the codecs' declarations say it -- the way tests/test_gpu_plan_ledger.py does for the U-Net.  Encode and decode outputs of each
case are compared with torch.equal.  What the parent did not reproduce bit for bit over two runs when the record was taken is listed
under "unstable" there and left to the fp64 gates (tests/test_gpu_codec_module_parity.py); every model and precision must keep at least
one stable tensor.  The record was taken on an MI355X and holds for that machine type.
"""
import json
import os

import numpy as np
import pytest
import torch

from tools import make_codec_pack_golden as mk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codec_pack_parent.npz")) as z:
        return json.loads(str(z["ledger"])), {k: torch.from_numpy(z[k]) for k in z.files if k != "ledger"}


@pytest.mark.parametrize("name", mk.CASES)
def test_codec_outputs_equal_the_build_before_the_named_layouts(golden, name):
    ledger, arrays = golden
    stored = sorted(k.split("/", 1)[1] for k in arrays if k.startswith(name + "/"))
    assert stored and set(stored) | set(ledger[name]["unstable"]) == {"encode", "decode"}
    got = mk.record(name)
    for k in stored:
        assert got[k].shape == arrays[f"{name}/{k}"].shape
        assert torch.equal(got[k], arrays[f"{name}/{k}"]), k
