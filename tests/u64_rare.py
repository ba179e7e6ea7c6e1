"""Shared by test_u64_rare_model.py and test_gpu_u64_rare_paths.py: the model
of the u64 kernels' lazy reduction (tests/golden/make_u64_rare_ids.py, loaded
from its file), the thresholds at both ends of every row of the u64 encode's
dispatch, and the degree range of the u64 baby-step/giant-step root test."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("make_u64_rare_ids",
                                               os.path.join(ROOT, "tests", "golden", "make_u64_rare_ids.py"))
rare = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rare)
P = rare.P

CHAIN_T = [2, 3, 5, 8, 13]
FOUR_T = [14, 16, 17, 20, 25, 28, 33, 36]
EIGHT_T = [21, 24, 29, 32, 37, 40, 41, 48, 49, 56, 57, 64, 65, 72, 73, 80]
PASS_T = [81, 88, 96, 160, 161, 168, 240, 300]


def rt64_bsgs_range():
    """(RT64_BSGS_MIND, RT64_BSGS_MAXD) of decode.hip."""
    src = open(os.path.join(ROOT, "sidekick_amd", "csrc", "decode.hip")).read()
    return tuple(int(re.search(r"constexpr uint32_t RT64_BSGS_%s = (\d+);" % k, src).group(1)) for k in ("MIND", "MAXD"))
