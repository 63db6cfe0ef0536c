"""What the two codecs' plan builders emit, against the record of the build before they were moved onto PlanBuilder's shared verbs
(csrc/plan.h conv_on / layer / bind_out / finalize / activated): tests/golden/codec_plan_parent.json (tools/make_codec_plan_golden.py, which
states the cases).

tests/test_gpu_codec_pack_ledger.py holds the codecs' OUTPUTS equal to the parent's; a launch reordered, dropped or given other arguments
that happen not to change the bits would pass there.  This holds the plans equal: every entry of the encode and the decode plan in order
-- kernel, module, FLOPs per sample, algorithmic bytes per sample and per launch, as doubles -- the launch count and flops_per_sample,
compared with ==, the way tests/test_gpu_plan_ledger.py does for the U-Net.  Nothing runs: the plans are reserved and their tables read.
Kernel names and byte counts do not encode the precision, so a model's bf16x3 record equals its fp32 record: the bf16x3 cases show that
switching the precision rebuilds the same plan, they discriminate nothing the fp32 cases do not (the split-bf16 operands are held by
tests/test_gpu_codec_pack_ledger.py, which compares what the plans compute).
The record was taken on an MI355X and holds for that machine type (tile choice depends on the CU count).
"""
import json
import os

import pytest

from tools import make_codec_plan_golden as mk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codec_plan_parent.json")) as f:
        return json.load(f)


def test_the_record_states_every_case(golden):
    assert sorted(golden) == sorted(mk.CASES)


@pytest.mark.parametrize("name", mk.CASES)
def test_codec_plans_equal_the_build_before_the_shared_verbs(golden, name):
    want, got = golden[name], mk.record(name)
    assert sorted(want) == sorted(got) == ["decode", "encode"]
    for op in ("encode", "decode"):
        w, g = want[op], got[op]
        assert len(w["entries"]) > 0 and w["launches"] == len(w["entries"])          # an empty record cannot pass
        assert g["launches"] == w["launches"] == len(g["entries"]), op
        for i, (ge, we) in enumerate(zip(g["entries"], w["entries"])):          # (the first difference by its index, before the whole lists)
            assert ge == we, (op, i)
        assert g["entries"] == w["entries"], op
        assert g["flops_per_sample"] == w["flops_per_sample"], op
