"""The row feed of the lane walk without a device: the interleaved copy's arithmetic and the rule of which targets take it
(csrc/lanes_plan.hpp: lane_rows_*, feed_is_rows), run in a small stand-alone program, and what the cross-compiled kernel looks like
(rh_grad_lane_kernel once more: a code object of its own next to the column feed's, under the report tag "lane_rows")."""
import os
import re
import subprocess
import tempfile

import pytest

from rainier_amd import _capi
from tests import lane_feed_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rainier_amd", "csrc")

# prints one line per query; the interleave runs on columns whose value tells where it came from: column j, row r -> 1000 (j + 1) + r
_MAIN = r'''
#include <cstdio>
#include <vector>
int main() {
  for (int nc = 1; nc <= 17; nc++)
    std::printf("eligible %d %d %d set %d %d\n", nc, (int)rh_plan::lane_rows_eligible(nc), (int)rh_plan::lane_rows_eligible(nc, 4),
                rh_plan::lane_rows_set(nc), rh_plan::lane_rows_set(nc, 4));
  const int ncs[] = {1, 2, 4, 8};
  const long long rowss[] = {1, 7, 8, 9, 17};
  for (int nc : ncs)
    for (long long rows : rowss) {
      std::vector<std::vector<double>> cols((size_t)nc, std::vector<double>((size_t)rows));
      std::vector<const double *> cp;
      for (int j = 0; j < nc; j++) {
        for (long long r = 0; r < rows; r++) cols[(size_t)j][(size_t)r] = 1000.0 * (j + 1) + (double)r;
        cp.push_back(cols[(size_t)j].data());
      }
      const long long n = rh_plan::lane_rows_doubles(rows, nc);
      std::vector<double> out((size_t)n + 2, -7.0);            // (a canary on either side of the copy)
      rh_plan::lane_rows_interleave(cp.data(), rows, nc, out.data() + 1);
      std::printf("copy %d %lld %lld %lld :", nc, rows, rh_plan::lane_rows_padded(rows), n);
      for (double v : out) std::printf(" %.0f", v);
      std::printf("\n");
      for (long long r = 0; r < rows; r++)
        for (int j = 0; j < nc; j++)
          if (out[(size_t)(1 + rh_plan::lane_rows_index(r, nc, j))] != 1000.0 * (j + 1) + (double)r) { std::printf("MISPLACED %d %lld %lld %d\n", nc, rows, r, j); return 1; }
    }
  std::printf("feed %d %d %d %d %d %d default %d\n", (int)rh_plan::feed_is_rows(true, 0), (int)rh_plan::feed_is_rows(true, 1), (int)rh_plan::feed_is_rows(true, 2),
              (int)rh_plan::feed_is_rows(false, 0), (int)rh_plan::feed_is_rows(false, 1), (int)rh_plan::feed_is_rows(false, 2), (int)rh_plan::kLaneFeedRowsDefault);
  {  // a launch may read the copies only if each holds the rows the launch walks (a copy is made from the rows that were uploaded;
     // data.nrows may name a prefix of them, never more)
    int dummy = 0;
    const void *copy[2] = {&dummy, nullptr};
    const long long have[2] = {1048613, 0};
    const long long full[2] = {5000000, 77}, prefix[2] = {1048613, 77}, shorter[2] = {63, 6}, none[2] = {0, 0};
    std::printf("cover %d %d %d %d %d\n", (int)rh_plan::lane_rows_cover(2, full, 2, have, copy), (int)rh_plan::lane_rows_cover(2, prefix, 2, have, copy),
                (int)rh_plan::lane_rows_cover(2, shorter, 2, have, copy), (int)rh_plan::lane_rows_cover(2, none, 2, have, copy),
                (int)rh_plan::lane_rows_cover(1, prefix, 2, have, copy));
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def plan():
    """the stand-alone program's output, line by line (built with the sanitizers of the host compiler: it has its own main)"""
    d = tempfile.mkdtemp(prefix="rh_lane_feed")
    src, exe = os.path.join(d, "feed.cpp"), os.path.join(d, "feed")
    open(src, "w").write('#include "%s"\n%s' % (os.path.join(CSRC, "lanes_plan.hpp"), _MAIN))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


def test_which_column_counts_take_the_row_feed_and_in_sets_of_how_many_rows(plan):
    got = {}
    for ln in plan:
        f = ln.split()
        if f[0] == "eligible":
            got[int(f[1])] = (int(f[2]), int(f[3]), int(f[5]), int(f[6]))
    assert sorted(got) == list(range(1, 18))
    # rows per set = min(rows per block, 16 / NC): 8, 8, 4, 2 with blocks of 8 rows; 4, 4, 4, 2 with blocks of 4
    assert {nc: got[nc] for nc in (1, 2, 4, 8)} == {1: (1, 1, 8, 4), 2: (1, 1, 8, 4), 4: (1, 1, 4, 4), 8: (1, 1, 2, 2)}
    for nc in (3, 5, 6, 7, 9, 10, 16, 17):
        assert got[nc][:2] == (0, 0), nc
    for nc in (1, 2, 4, 8):
        for set_rows, block in ((got[nc][2], 8), (got[nc][3], 4)):
            assert 2 * set_rows * nc * 2 <= 64        # two sets in the 64 scalar registers the column feed holds
            assert block % set_rows == 0 and 8 % set_rows == 0      # whole sets per block, and per block of the padding
            nbytes = set_rows * nc * 8                # one or two whole 64-byte lines; half a line for one column in blocks of 4 rows
            assert nbytes in (64, 128) or (block == 4 and nc == 1 and nbytes == 32)


def test_the_interleaved_copy_has_every_element_in_its_place_and_zeros_behind(plan):
    seen = []
    for ln in plan:
        assert not ln.startswith("MISPLACED"), ln
        if not ln.startswith("copy"):
            continue
        head, vals = ln.split(" :")
        nc, rows, padded, n = (int(x) for x in head.split()[1:])
        vals = [float(v) for v in vals.split()]
        seen.append((nc, rows))
        assert padded == (rows + 7) // 8 * 8 and padded % 8 == 0 and 0 <= padded - rows < 8 and n == padded * nc
        assert vals[0] == -7.0 and vals[-1] == -7.0 and len(vals) == n + 2        # nothing written outside the copy
        body = vals[1:-1]
        for r in range(rows):
            for j in range(nc):
                assert body[r * nc + j] == 1000.0 * (j + 1) + r
        assert all(v == 0.0 for v in body[rows * nc:]) and len(body[rows * nc:]) == (padded - rows) * nc
    assert seen == [(nc, rows) for nc in (1, 2, 4, 8) for rows in (1, 7, 8, 9, 17)]


def test_the_knob_forces_the_feed_and_rows_falls_back_where_there_is_no_kernel(plan):
    f = [ln.split() for ln in plan if ln.startswith("feed")][0]
    default = int(f[8])
    assert [int(x) for x in f[1:7]] == [default, 0, 1, 0, 0, 0]
    assert default == 1          # the row feed is the choice wherever the kernel exists (profiles/lane_feed_cfg2)


def test_a_launch_reads_a_copy_only_if_the_copy_holds_its_rows(plan):
    # a copy of 1 048 613 rows (a prefix the create-time self-check evaluates) must not serve a launch over 5 000 000; a target
    # without a copy walks its columns whatever its length; the counts of targets must agree
    f = [ln.split() for ln in plan if ln.startswith("cover")][0]
    assert [int(x) for x in f[1:]] == [0, 1, 1, 1, 0]


# ---- the cross-compile report of every case (tests/lane_feed_cases.py), with the case's data ----
_reports = {}


def _report(case):
    if case.name not in _reports:
        spec = case.make(FC.N_BUILD)
        _reports[case.name] = _capi.lower_report(spec.rir, _capi.compile_opts(**case.opts), columns=spec.columns, nrows=spec.nrows)
    return _reports[case.name]


def _tag(rep, tag):
    return {k: v for (t, k), v in rep["kernels"].items() if t == tag}


@pytest.mark.parametrize("case", FC.CASES, ids=repr)
def test_which_models_get_the_row_fed_kernel(case):
    src, rep = _report(case)
    lane, rows = _tag(rep, "lane"), _tag(rep, "lane_rows")
    assert max(int(x) for x in re.findall(r"NCOLS = (\d+)", src)) == case.nc       # (the data-free target has none)
    # the "lane" tag is what it was: exactly the column-fed kernel, or nothing
    assert list(lane) == ([FC.LANE] if case.cols else [])
    base = {k for (t, k) in rep["kernels"] if t == "base"}
    assert FC.LANE not in base and FC.LANE not in src and "RH_LANE_FEED_ROWS" not in src
    if not case.rows and case.why is None:
        assert not rows, (case, rows)         # no eligible target (or no lane walk at all): nothing was built
        return
    assert list(rows) == [FC.LANE]
    k, c = rows[FC.LANE], lane[FC.LANE]
    if not case.rows:
        assert not k["fit"] and case.why in k["why"], k
        return
    assert k["fit"] and k["vgpr_spills"] == 0 and k["sgpr_spills"] == 0 and k["scratch"] == 0 and k["unproven"] == 0
    assert k["lds"] == c["lds"] and k["lane_r"] == c["lane_r"]        # the same sums through LDS, the same blocks of rows
    assert 0 < k["vgprs"] <= c["vgprs"]
    if c["vgprs"] <= 64:
        assert k["vgprs"] <= 64               # eight wavefronts per SIMD where the column feed has them
    if case.name == "linreg3-strict":         # cfg 2's strict build: 74 against the column feed's 98 -- six wavefronts per SIMD (the
        assert c["vgprs"] > 80 and 64 < k["vgprs"] <= 80      # granule is 8 registers) where the column feed has five; LDS allows six


def test_the_flagship_build_keeps_eight_wavefronts_per_simd_under_the_row_feed():
    for build, block in (("fast", 8), ("strict", 4)):
        _, rep = _report(FC.BY_NAME["linreg3-%s" % build])
        k, c = _tag(rep, "lane_rows")[FC.LANE], _tag(rep, "lane")[FC.LANE]
        assert k["fit"] and k["lane_r"] == block and k["lds"] == c["lds"]
    _, rep = _report(FC.BY_NAME["linreg3-fast"])
    k = _tag(rep, "lane_rows")[FC.LANE]
    assert k["vgprs"] <= 64 and k["sgprs"] <= 104 and k["lds"] == 40960
