"""The small device forms every walk loop is built from (csrc/vr_device.h: f2i, f2u, lshl_or,
bit_select, bit_sel, Ctx::cell, word_index, word_offset, word_bit5, word_bit5c) against plain C
formulas on the host.  bin/walk_words_check (csrc/tools/walk_words_check.hip) runs one lane per
case and prints the counts asserted here:

  cells   : all 64^3 integer cells of a region -- the in-loop conversion (the plain cast, which
            must be f2i there), the mask word's index, its byte offset from the region's base
            (shift 3 and 2) and the voxel's bit in the word's low five bits;
  frac    : the same for 200 000 seeded positions in [0, 64) plus 408 with +0, 63.999996 and the
            floats next to every integer on an axis;
  cvt     : f2i / f2u at NaN, +-0, +-inf, +-2^31, 2^31 - 128, -2^31 - 256, denormals, +-63.5,
            64.0, 2^32 and 100 000 seeded bit patterns (truncate, saturate, NaN -> 0);
  select  : bit_select and bit_sel for masks 0 and ~0 (50 000 operand pairs each);
  lshl_or : the shifts the walks use (1, 3, 4, 10), 50 000 operand pairs.

One small launch per group: the tool runs well under a second."""
from __future__ import annotations

import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "voxelraymarcher_amd", "bin", "walk_words_check")


@pytest.mark.gpu
def test_walk_words_match_plain_formulas():
    assert os.path.exists(EXE), "build with make -C voxelraymarcher_amd/csrc"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode in (0, 1), r.stderr              # anything else: it crashed
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    assert res["cells"] == 64 ** 3
    assert res["frac_edge"] == 408 and res["frac"] == 200_000 + res["frac_edge"]
    assert res["cvt_named"] == 23 and res["cvt"] == 100_000 + res["cvt_named"]
    assert res["select"] == 100_000
    assert res["lshl_or"] == 50_000 and res["lshl_or_shifts"] == 4
    for k in ("cells_bad", "frac_bad", "cvt_bad", "select_bad", "lshl_or_bad"):
        assert res[k] == 0, (k, res, r.stderr)
    assert res["ok"] is True and r.returncode == 0
