"""CPU: TW_OPT_ROLLOUT_DRAIN (the hand-over of the persistent 256-episode f32 rollout) is accepted and refused as include/twisterl_hip.h
documents it, and the header, twisterl_amd/_lib.py and docs/hip.rs give it the same number.  Needs no device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_option_has_one_number_everywhere():
    from twisterl_amd import _lib
    header = open(os.path.join(ROOT, "include", "twisterl_hip.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(TW_OPT_[A-Z0-9_]+) = (\d+)", header))
    assert enum["TW_OPT_ROLLOUT_DRAIN"] == 9 == max(enum.values())                       # the next free number (7 stays unassigned)
    assert len(set(enum.values())) == len(enum)
    assert enum == {k: getattr(_lib, k) for k in dir(_lib) if k.startswith("TW_OPT_")}
    rs = open(os.path.join(ROOT, "docs", "hip.rs")).read()
    assert re.search(r"const TW_OPT_ROLLOUT_DRAIN: c_int = (\d+);", rs).group(1) == "9"


def test_values_are_accepted_and_refused_as_documented():
    from twisterl_amd import _lib
    lib = _lib.lib()
    opt = _lib.TW_OPT_ROLLOUT_DRAIN
    try:
        for v in (0, -1, 1, 32, 128, 256):                       # automatic, off, live episodes per workgroup
            assert lib.tw_set_launch_option(opt, v) == _lib.TW_OK, v
        for v in (-2, 257, 1 << 20):
            assert lib.tw_set_launch_option(opt, v) == _lib.TW_ERR_INVALID, v
            assert b"TW_OPT_ROLLOUT_DRAIN" in lib.tw_last_error()
        assert lib.tw_set_launch_option(7, 0) == _lib.TW_ERR_INVALID and lib.tw_set_launch_option(10, 0) == _lib.TW_ERR_INVALID
    finally:
        assert lib.tw_set_launch_option(opt, 0) == _lib.TW_OK
