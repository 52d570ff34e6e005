"""tools/box_atomic_depth.py: the CPU model of one box atomic wave instruction of blur_mfma_kernel<SCORE> (no GPU).

Pins what the live-lane predicate rests on: how deep the ds_add_u32 of a wave serialise with all 64 lanes issuing and with the
live lanes only and the share of lanes that are not live -- and what the model says of the table row pitch (the kernel's is
16 (nbx + 1); choose_pitch is the model's answer to "which pitch would be conflict-free", kept as a measurement)."""
import importlib.util
import os

import pytest

_spec = importlib.util.spec_from_file_location(
    "box_atomic_depth", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "box_atomic_depth.py"))
model = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(model)

_reports = {}


def _report(w, h):
    if (w, h) not in _reports:
        _reports[(w, h)] = model.report(w, h, 272)
    return _reports[(w, h)]


def test_4k_dead_lanes_double_the_chain():
    r = _report(3840, 2160)
    assert (r["nbx"], r["nby"]) == (10, 38)
    assert r["all"][0] == pytest.approx(4.0, abs=0.005)          # same dword, all lanes
    assert r["live"][0] == pytest.approx(2.0, abs=0.005)         # ... live lanes only
    assert r["live"][1] == pytest.approx(2.0, abs=0.005)         # and no bank conflict beyond it
    assert r["all"][1] > 4.0                                     # the spare column's banks on top
    assert r["dead"] == pytest.approx(28 / 64, abs=1e-9)         # lane 15 + slots 3 and 4: 44 %
    assert round(100 * r["dead"]) == 44


def test_4k_pitch_comes_out_unchanged():
    r = _report(3840, 2160)
    assert r["pitch"] == r["pitch_min"] == 16 * 11
    assert r["live_at_pitch"] == pytest.approx(r["live"])


def test_8k_dead_lane_share():
    r = _report(7680, 4320)
    assert r["dead"] == pytest.approx(40 / 64, abs=1e-9)         # two slots live: 10 of 16 lanes dead, 62 %
    assert round(100 * r["dead"] - 0.01) == 62
    assert r["all"][0] == pytest.approx(3 * r["live"][0], rel=0.01)
    assert r["pitch"] == r["pitch_min"]


@pytest.mark.parametrize("w,h", [(2560, 1440), (2200, 1238)])
def test_small_boxes_pitch_or_no_room(w, h):
    """the table pitch hides nothing here: live lanes conflict on banks four deep at a same-dword depth under two.  Either the
    chosen pitch brings the bank depth down to the dword depth, or no pitch fits beside three workgroups' LDS"""
    r = _report(w, h)
    assert r["live"][1] > r["live"][0] + 1.0
    if r["pitch"] is None:
        geo = model.Geometry(w, h, 272)
        assert 2 * geo.min_pitch() * (geo.nby + 1) > model.lds_budget()    # today's tables alone are past the budget
    else:
        assert r["pitch"] % 16 == 0 and r["pitch"] >= r["pitch_min"]
        assert 2 * r["pitch"] * (r["nby"] + 1) <= model.lds_budget()
        assert r["live_at_pitch"][1] == pytest.approx(r["live_at_pitch"][0], abs=1e-9)


def test_short_segments_at_1440p_get_a_padded_pitch():
    """a single 1440p image marches short segments: the tables would fit, and the model pads the pitch from 60 to 80 words"""
    r = model.report(2560, 1440, 128)
    assert r["pitch_min"] == 240 and r["pitch"] == 320
    assert r["live"][1] == pytest.approx(4.0, abs=0.005)
    assert r["live_at_pitch"][1] == pytest.approx(r["live_at_pitch"][0], abs=1e-9)
    assert r["live_at_pitch"][0] == pytest.approx(r["live"][0])
