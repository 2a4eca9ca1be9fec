#!/usr/bin/env python3
"""How often does the reference's longest_match_c / longest_match_slow_c depend on how the reference was built?

Runs the in-contract corpus of tests/test_oracle_ref_prims.py (every window size, data kind, phase, cur_match candidate
and (prev_length, lookahead) pair) through both builds under oracle/_ref: the byte-compare one (NO_UNALIGNED,
OPTIMAL_CMP 8; the one the oracle and the kernels are pinned to) and the build host's default, and counts per level the
calls whose (length, match_start) differ.  A measurement for DESIGN.md section 1: nothing asserts on the native build.

    python tools/ref_variant_diff.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib                                                                                    # noqa: E402
from deflate_state_util import (DATA_KINDS, WINDOW_SIZES, cur_match_candidates, in_contract_snapshots,   # noqa: E402
                                match_call, match_param_sets, set_match_level)


def main():
    pin, native = oracle_lib.load_ref_prims("bytecmp"), oracle_lib.load_ref_prims("native")
    print("OPTIMAL_CMP: pinned build %d, native build %d" % (pin.ref_optimal_cmp(), native.ref_optimal_cmp()))
    calls, diffs, len_diffs = {}, {}, {}
    for w_size in WINDOW_SIZES:
        for kind in DATA_KINDS:
            for roll, fast_levels, slow_levels in ((False, range(1, 9), (7, 8)), (True, (9,), (9,))):
                for snap in in_contract_snapshots(pin, "ref_", kind, w_size, roll, per_phase=6):
                    curs = cur_match_candidates(snap, kind, roll)
                    for name, levels in (("longest_match", fast_levels), ("longest_match_slow", slow_levels)):
                        a, b = getattr(pin, "ref_" + name), getattr(native, "ref_" + name)
                        for level in levels:
                            set_match_level(snap, level)
                            key = (name, level)
                            for cur in curs:
                                for p, la in match_param_sets(level):
                                    x, y = match_call(a, snap, cur, p, la), match_call(b, snap, cur, p, la)
                                    calls[key] = calls.get(key, 0) + 1
                                    diffs[key] = diffs.get(key, 0) + (x != y)
                                    len_diffs[key] = len_diffs.get(key, 0) + (x[0] != y[0])
    print("%-20s %5s %8s %8s %10s" % ("function", "level", "calls", "differ", "length"))
    for key in sorted(calls):
        print("%-20s %5d %8d %8d %10d" % (key[0], key[1], calls[key], diffs[key], len_diffs[key]))


if __name__ == "__main__":
    main()
