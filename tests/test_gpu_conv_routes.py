"""The instantiation every pipelined convolution launch runs on, against the record of the build before the instantiation table
(conv_pipe.hip conv_pipe_select), tests/golden/conv_routes_parent.json (tools/make_conv_routes_golden.py).

Routing is host logic: which conv_pipe_kernel instantiation a launch goes to is a function of its shapes, the plan's form and the
runtime's occupancy answers.  Each case of the tool is rerun here and must reproduce, exactly and in order, the plan's entry kernel names
(`+fin`: what the occupancy query decided), the thirteen template arguments of every launch's instantiation (fc_debug_conv_routes) and
the step-route record -- inference plans exclusive and shared, replayed Euler steps on the step-closing flavour, a dim-16 model's
run-time-geometry flavours, a training step, the mask path, and both codecs (the SD-VAE also in split-bf16).  76 of the 197
instantiations are launched.  No case this small fills the grids of the 64-column tiles: of M128N64 only the all-in-one 1x1 kernel
is in the record, of M256N64 nothing, and the split-bf16 rows are those of M128N32.  The record was
taken on an MI355X and holds for that machine type: occupancy, tile choice and the mask case's batch depend on its CU count.
"""
import json
import os

import pytest

from tools import make_conv_routes_golden as mk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes_parent.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(mk.CASES))
def test_routes_equal_the_build_before_the_table(golden, name):
    got, want = mk.record(name), golden[name]
    assert got["kernels"] == want["kernels"]
    assert got["steps"] == want["steps"]
    assert len(want["launches"]) > 0
    assert [got["instantiations"][i] for i in got["launches"]] == [want["instantiations"][i] for i in want["launches"]]
