"""The tap-major GEMM engine's launch decisions, on the host: every query of
tools/conv_launch_table.py answers what it answered before the policy moved
into conv_t_launch.h (tests/golden/conv_launch_table.json, generated from that
commit), and a clip-norm weight gradient refuses a short workspace or slot row
before any device work."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT
from flr import _capi


def _tool():
    spec = importlib.util.spec_from_file_location("conv_launch_table", os.path.join(ROOT, "tools", "conv_launch_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "conv_launch_table.json")) as fh:
        return TOOL.unpack(json.load(fh))  # stored without its repeated rows


def _assert_same(got, want, label):
    assert got.keys() == want.keys(), label
    for part in want:
        assert got[part].keys() == want[part].keys(), (label, part)
        for key, value in want[part].items():
            assert got[part][key] == value, (label, part, key)


def test_table_covers_the_settings(golden):
    assert list(golden) == [label for label, _, _ in TOOL.SETTINGS]
    assert len(golden["default"]["conv"]) == len(TOOL.SHAPES) * len(TOOL.CLIENTS) * len(TOOL.BATCHES)


def test_decisions_match_the_pinned_table(golden):
    got = TOOL.table()
    assert list(got) == list(golden)
    for label in golden:
        _assert_same(got[label], golden[label], label)


@pytest.mark.parametrize("name", ["FLR_CONV_MINKT", "FLR_BGEMM_MINKT", "FLR_DGRAD_MINKT1", "FLR_DGRAD_MINKT2"])
def test_removed_tuning_knobs_change_nothing(golden, knob, name):
    knob(name, 4)
    _assert_same(TOOL.table_for_current_knobs(), golden["default"], name)


# one conv of layer 1 at 4 clients: the weight gradient splits K (workspace > 0)
GEO = (4, 32, 64, 8, 8, 64, 3, 3, 1, 1)
DUMMY = 0x1000  # never dereferenced: every call below is refused on the host


def _wgrad_sq(sq_ld, ws, ws_bytes):
    return _capi.lib().flr_conv2d_bwd_weight_t_sq(DUMMY, DUMMY, DUMMY, *GEO, 0, DUMMY, sq_ld, ws, ws_bytes, None)


def test_clip_norm_wgrad_refuses_short_workspace_or_slots():
    lib = _capi.lib()
    ws = int(lib.flr_conv2d_t_workspace(*GEO))
    slots = int(lib.flr_conv2d_bwd_weight_t_sq_slots(*GEO))
    assert ws > 0 and slots > 0
    assert _wgrad_sq(slots, DUMMY, ws - 1) == _capi.FLR_ERR_WORKSPACE
    assert _wgrad_sq(slots - 1, DUMMY, ws) == _capi.FLR_ERR_WORKSPACE
    assert _wgrad_sq(slots, None, ws) == _capi.FLR_ERR_WORKSPACE
