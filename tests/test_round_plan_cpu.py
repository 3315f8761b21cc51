"""The rounds of a tick-engine run as arithmetic (csrc/lanes_plan.hpp round_launches / round_cap: how many gradient launches
csrc/engine.cpp advance_to_ticks enqueues on a lane before it synchronises and asks how many chains still run), called through a tiny
host library and compared with literals worked by hand; and the same header once more in a small stand-alone program built with the
host compiler's sanitizers, which plays whole runs the way the engine does and prints every round.

The rule: a lock-step run (static HMC in the sampling phase, whose count of launches still to do is exact) takes its whole remainder
in one round, up to the cap -- 4096, or what RH_ROUND_MAX lowers it to --; everything else asks after 32 launches and never enqueues
more than 256."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rainier_amd", "csrc")

_WRAP = r'''
extern "C" int rp_round(int lock_step, long long remaining, int ltraj, int cap) { return rh_plan::round_launches(lock_step != 0, remaining, ltraj, cap); }
extern "C" int rp_cap(int requested) { return rh_plan::round_cap(requested); }
extern "C" void rp_consts(int *out) { out[0] = rh_plan::kRoundCapDefault; out[1] = rh_plan::kRoundMaxDynamic; out[2] = rh_plan::kRoundHint; }
'''
_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="rh_round_plan")
        src, so = os.path.join(d, "plan.cpp"), os.path.join(d, "plan.so")
        open(src, "w").write('#include "%s"\n%s' % (os.path.join(CSRC, "lanes_plan.hpp"), _WRAP))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", so])
        L = C.CDLL(so)
        L.rp_round.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_int]
        _lib = L
    return _lib


def rounds(remaining, ltraj, cap, lock_step=True):
    """the rounds of a lock-step run of `remaining` launches, as the engine takes them: plan, enqueue, subtract"""
    out = []
    while remaining > 0:
        out.append(lib().rp_round(int(lock_step), remaining, ltraj, cap))
        assert out[-1] >= 1
        remaining -= out[-1]
    assert remaining == 0
    return out


def test_the_constants():
    out = (C.c_int * 3)()
    lib().rp_consts(out)
    assert list(out) == [4096, 256, 32]


def test_a_lock_step_run_is_one_round_up_to_the_cap():
    assert rounds(2048, 32, 4096) == [2048]                     # the flagship: 64 iterations x L = 32 per lane
    assert rounds(10_000, 32, 4096) == [4096, 4096, 1808]
    assert rounds(4096, 32, 4096) == [4096] and rounds(4097, 32, 4096) == [4096, 1]
    assert rounds(36, 4, 4096) == [36]


def test_a_low_cap_ends_rounds_in_mid_trajectory_at_both_parities():
    """cap 5 with L = 4: the rounds of 36 launches end behind launches 5, 10, 15, 20, ... -- positions 1, 2, 3, 0 of a trajectory,
    and an odd and an even number of launches into the partial-sum ping-pong alternately"""
    got = rounds(36, 4, 5)
    assert got == [5, 5, 5, 5, 5, 5, 5, 1]
    ends = [sum(got[:k + 1]) for k in range(len(got))]
    assert [e % 4 for e in ends[:4]] == [1, 2, 3, 0] and {e % 2 for e in ends} == {0, 1}
    assert rounds(36, 4, 3) == [3] * 12 and rounds(36, 4, 7) == [7, 7, 7, 7, 7, 1] and rounds(36, 4, 1) == [1] * 36


def test_everything_else_keeps_32_and_256():
    r = lib().rp_round
    assert r(0, 32, 4, 4096) == 32                              # the hint the engine passes for warm-up, EHMC and NUTS
    assert r(0, 10_000, 4, 4096) == 256 and r(0, 256, 4, 4096) == 256 and r(0, 257, 4, 4096) == 256 and r(0, 255, 4, 4096) == 255
    assert r(0, 32, 4, 3) == 3 and r(0, 32, 4, 64) == 32        # the cap binds here too
    assert r(0, 0, 4, 4096) == 1 and r(0, -5, 4, 4096) == 1


def test_remaining_zero_or_one():
    r = lib().rp_round
    assert r(1, 1, 32, 4096) == 1
    # a lock-step count that has run out while a chain still runs is no longer exact: one trajectory at a time
    assert r(1, 0, 32, 4096) == 32 and r(1, 0, 4, 4096) == 4 and r(1, 0, 4, 3) == 3 and r(1, -1, 0, 4096) == 1


def test_a_cap_below_one_reads_as_one():
    r = lib().rp_round
    for cap in (0, -1, -4096):
        assert r(1, 2048, 32, cap) == 1 and r(0, 32, 32, cap) == 1 and r(1, 0, 32, cap) == 1
    c = lib().rp_cap
    assert [c(n) for n in (-3, 0, 1, 3, 4095, 4096, 4097, 1 << 30)] == [1, 1, 1, 3, 4095, 4096, 4096, 4096]


# ---- the same header under the host sanitizers: whole runs, played as the engine plays them ----
# one line per run: "run <lock> <todo> <ltraj> <cap> : <round> <round> ..."; the program keeps the engine's own books (launches still
# to do, position in the trajectory, a was-ticked slot per launch of a round in an array of exactly `cap` entries with a canary
# behind it) and fails if a round is longer than the cap or the array is overrun
_MAIN = r'''
#include <cstdio>
#include <vector>
static int play(bool lock_step, long long todo, int ltraj, int cap_req, bool capped) {
  const int cap = capped ? rh_plan::round_cap(cap_req) : rh_plan::kRoundCapDefault;
  std::vector<char> was_ticked((size_t)cap + 1, 0);
  was_ticked[(size_t)cap] = 77;
  std::printf("run %d %lld %d %d :", (int)lock_step, todo, ltraj, cap);
  long long remaining = todo, pos = 0, budget = todo;
  for (int round = 0; (lock_step ? remaining > 0 : budget > 0) && round < 100000; round++) {
    const int B = rh_plan::round_launches(lock_step, lock_step ? remaining : rh_plan::kRoundHint, ltraj, cap);
    if (B < 1 || B > cap) { std::printf(" BAD %d\n", B); return 1; }
    for (int i = 0; i < B; i++, pos++) was_ticked[(size_t)i] = (pos % ltraj) + 1 == ltraj || i == B - 1;
    std::printf(" %d", B);
    if (lock_step) remaining -= B; else budget -= B;
  }
  std::printf("\n");
  return was_ticked[(size_t)cap] == 77 && (!lock_step || remaining == 0) ? 0 : 1;
}
int main() {
  int bad = 0;
  bad += play(true, 2048, 32, 0, false);
  bad += play(true, 10000, 32, 0, false);
  bad += play(true, 36, 4, 5, true);
  bad += play(true, 7, 4, 3, true);
  bad += play(true, 36, 4, -2, true);
  bad += play(true, 1, 4, 1 << 30, true);
  bad += play(false, 100, 4, 0, false);
  bad += play(false, 10, 4, 3, true);
  return bad ? 1 : 0;
}
'''


@pytest.fixture(scope="module")
def runs():
    d = tempfile.mkdtemp(prefix="rh_round_plan_san")
    src, exe = os.path.join(d, "rounds.cpp"), os.path.join(d, "rounds")
    open(src, "w").write('#include "%s"\n%s' % (os.path.join(CSRC, "lanes_plan.hpp"), _MAIN))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    return {tuple(int(x) for x in ln.split(" :")[0].split()[1:]): [int(x) for x in ln.split(" :")[1].split()] for ln in out}


def test_whole_runs_under_the_host_sanitizers(runs):
    assert runs == {
        (1, 2048, 32, 4096): [2048],
        (1, 10000, 32, 4096): [4096, 4096, 1808],
        (1, 36, 4, 5): [5, 5, 5, 5, 5, 5, 5, 1],
        (1, 7, 4, 3): [3, 3, 1],
        (1, 36, 4, 1): [1] * 36,
        (1, 1, 4, 4096): [1],
        (0, 100, 4, 4096): [32, 32, 32, 32],
        (0, 10, 4, 3): [3, 3, 3, 3],
    }
