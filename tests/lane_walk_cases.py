"""The models the lane walk of the gradient row loop (rh_grad_lane_kernel, csrc/device/rh_lane.hip.h) is tested on beyond linreg with
three covariates, shared by the cross-compile checks (tests/test_lane_walk_cpu.py), the device tests
(tests/test_gpu_lane_walk_models.py) and build() (__graft_entry__.py build_jobs, so that the device tests compile nothing).  No device
is needed here.

A case is (name, spec factory, opts, expected R, expected lane): `make(n, npoints)` -> (spec, points | None) builds the model on n
rows -- an int, or (n1, n2) for the models with two row targets --; `r` is the rows per scalar request the engine settles on
(8, or 4 where the row code leaves too few scalar registers for 8), `lane` whether the model gets a lane kernel at all.  What is
expected here was read off the cross-compile reports (_capi.lower_report); tests/test_lane_walk_cpu.py holds every line to them, so
a model that silently loses -- or gains -- the walk is noticed."""
import numpy as np

from rainier_amd import _capi, models
from rainier_amd.frontend import Graph
from tests.fuzz_models import GPU_FUZZ_CASES, eight_slot_model, gpu_fuzz_case

FAST = dict(fp_contract=True, factor_outputs=True)
STRICT = dict(math_mode=_capi.MATH_STRICT)
BUILDS = {"fast": FAST, "strict": STRICT}

# the row counts every case is run at: around the block of R = 8 and of R = 4 rows (a target shorter than one block, exactly one,
# one and a ragged row), around the 512 rows of 8 wavefronts x 8 splits x 8 rows, and a count that is ragged against all of them
ROW_COUNTS = (1, 3, 4, 5, 8, 9, 511, 513, 4099)
ROW_COUNTS_2 = ((1037, 5), (5, 1037), (8, 8), (4099, 1))
N_MAIN, N_MAIN_2 = 4099, (1037, 5)      # where the chain counts and the row splits are varied
N_BUILD, N_BUILD_2 = 9, (8, 8)          # what build() lowers (the generated source does not depend on the row count)


def two_targets(n, seed=31):
    """linreg with one covariate and a second likelihood of its own: theta = (s, a, b), linreg's prior, y | x ~ N(a + b x, e^s)
    over n1 rows of (y, x) -- without the constant --, and z ~ N(b, 1) over n2 rows of z"""
    n1, n2 = n
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n1)
    y = 0.5 + 1.5 * x + 0.7 * rng.standard_normal(n1)
    z = 1.5 + rng.standard_normal(n2)
    g = Graph(3, [0, 2, 1])
    s, a, b = g.param(0), g.param(1), g.param(2)
    prior = (s - s.exp()) + models.std_normal_logpdf(a) + models.std_normal_logpdf(b)
    r = g.col(1, 0) - (a + b * g.col(1, 1))
    t1 = r * r * (s * -2.0).exp() / -2.0 - s
    d = g.col(2, 0) - b
    t2 = d * d * -0.5
    return models.ModelSpec("two_targets_%dx%d" % (n1, n2), g.compile([prior, t1, t2]), [y, x, z], [0, n1, n2], 3, {"kind": "two_targets"})


def two_targets_log(n, seed=32):
    """two row targets of one column each and no data-free one: theta = (a, b), c1 ~ N(a, 1) and a Cauchy-shaped term in c2 - a b"""
    n1, n2 = n
    rng = np.random.default_rng(seed)
    c1 = 0.4 + rng.standard_normal(n1)
    c2 = rng.standard_normal(n2) * 1.5
    g = Graph(2, [0, 1, 1])
    a, b = g.param(0), g.param(1)
    d1 = g.col(1, 0) - a
    d2 = g.col(2, 0) - a * b
    # (target 0 carries no rows: the standard normal prior of a and b)
    prior = models.std_normal_logpdf(a) + models.std_normal_logpdf(b)
    return models.ModelSpec("two_targets_log_%dx%d" % (n1, n2), g.compile([prior, d1 * d1 * -0.5, -((d2 * d2 + 1.0).log())]), [c1, c2],
                            [0, n1, n2], 2, {"kind": "two_targets_log"})


def _fit_normal(n):
    return models.fit_normal(np.random.default_rng(33).normal(1.5, 0.8, size=n))


class Case:
    def __init__(self, name, make, build, r, lane, value_only=False, targets=1, rows=None, n_build=None):
        self.name, self._make, self.build, self.opts, self.r, self.lane = "%s-%s" % (name, build), make, build, BUILDS[build], r, lane
        self.value_only = value_only        # the build has a value-only part: row_g() differs from row()
        self.targets = targets              # row targets
        self.fuzz = name.startswith("slots")
        self._rows, self._n_build = rows, n_build

    def make(self, n, npoints=0):
        """-> (spec, points): `npoints` finite evaluation points -- rng.normal(0, 0.6), or those the fuzz generator returns"""
        if self.fuzz:
            spec, qs = self._make(n, npoints)
            if npoints:
                qs = np.resize(np.asarray(qs), (npoints, spec.n_params))     # (fewer finite points than asked for: repeated)
            return spec, qs
        spec = self._make(n)
        return spec, np.random.default_rng(20).normal(0.0, 0.6, size=(npoints, spec.n_params))

    @property
    def row_counts(self):
        return self._rows or (ROW_COUNTS if self.targets == 1 else ROW_COUNTS_2)

    @property
    def n_main(self):
        return N_MAIN if self.targets == 1 else N_MAIN_2

    @property
    def n_build(self):
        return self._n_build or (N_BUILD if self.targets == 1 else N_BUILD_2)

    def __repr__(self):
        return self.name


def _linreg(k):
    return lambda n: models.linreg(n=n, k=k)


def _slots(seed):
    """the eight-slot random model of tests/fuzz_models.GPU_FUZZ_CASES with this seed -- its random expression depends on its row
    count, so the program and the points are those of that case -- on n rows of data of the same make: (x, z, -x) per slot"""
    def make(n, npoints=0):
        spec, qs = eight_slot_model(seed, n=dict(FUZZ_SLOTS)[seed]["n"], npoints=npoints)
        rng = np.random.default_rng(5000 + seed)
        cols = []
        for _ in range(8):
            x = rng.uniform(-1, 1, n)
            cols += [x, rng.uniform(-1, 1, n), -x]
        return models.ModelSpec("%s_x%d" % (spec.name, n), spec.rir, cols, [n], spec.n_params, {}), qs
    return make


# the "slots" cases of tests/fuzz_models.GPU_FUZZ_CASES, as (seed, keywords)
FUZZ_SLOTS = [(seed, kw) for kind, seed, kw in GPU_FUZZ_CASES if kind == "slots"]
# The eight slots are rolled into ONE row target of 2 columns and 8 n rows -- the shape the lane walk fits -- from 3 rows per slot on
# in a fast build and from some count between 10 and 16 on in a strict one; below that the program keeps its 24 columns, is another
# source and has no lane kernel.  So these cases run at the row counts of the others that roll (the kernel walks 8 n rows).
SLOTS_ROWS = {"fast": dict(rows=ROW_COUNTS[1:], n_build=16), "strict": dict(rows=(16, 17) + ROW_COUNTS[6:], n_build=16)}

POSITIVE = [
    Case("linreg1", _linreg(1), "fast", 8, True),                               # NACC 3 of RH_NACC_MAX 3, NINV 4
    Case("linreg1", _linreg(1), "strict", 8, True, value_only=True),
    Case("fit_normal", _fit_normal, "fast", 8, True, value_only=True),          # one column; row_g() in a fast build
    Case("fit_normal", _fit_normal, "strict", 8, True, value_only=True),
    Case("linreg4", _linreg(4), "fast", 4, True),                               # 5 columns: R = 4 in a fast build
    Case("linreg5", _linreg(5), "strict", 4, True, value_only=True),            # NACC 8: 64 KB of static LDS
    Case("linreg6", _linreg(6), "fast", 4, True),                               # NACC 8, 7 columns
] + [Case("slots%d" % s, _slots(s), "fast", 8, True, value_only=s > 0, **SLOTS_ROWS["fast"]) for s in (0, 2, 3)] + [     # row code of up to 230 VGPRs
    Case("slots0", _slots(0), "strict", 8, True, value_only=True, **SLOTS_ROWS["strict"]),
    Case("slots2", _slots(2), "strict", 8, True, value_only=True, **SLOTS_ROWS["strict"]),                                # 254 VGPRs
    Case("two_targets", two_targets, "fast", 8, True, value_only=True, targets=2),               # NACC 3-4 and 1-2: NA < RH_NACC_MAX in the second
    Case("two_targets", two_targets, "strict", 8, True, value_only=True, targets=2),
    Case("two_targets_log", two_targets_log, "fast", 8, True, value_only=True, targets=2),
    Case("two_targets_log", two_targets_log, "strict", 8, True, value_only=True, targets=2),
]

NEGATIVE = [
    Case("linreg7", _linreg(7), "fast", 0, False),                              # NACC 9: 72 KB of LDS
    Case("linreg7", _linreg(7), "strict", 0, False),
    Case("linreg6", _linreg(6), "strict", 0, False),                            # NACC 9 in the strict build
    Case("logistic2", lambda n: models.logistic(n=n, k=2), "fast", 0, False),
    Case("logistic2", lambda n: models.logistic(n=n, k=2), "strict", 0, False),
    Case("negbin_glm", lambda n: models.negbin_glm(n=n), "fast", 0, False),
    Case("negbin_glm", lambda n: models.negbin_glm(n=n), "strict", 0, False),
    Case("slots1", _slots(1), "fast", 0, False, n_build=16),
] + [Case("slots%d" % s, _slots(s), "strict", 0, False, n_build=16) for s in (1, 3)]

CASES = POSITIVE + NEGATIVE

# the "slots" cases of tests/fuzz_models.GPU_FUZZ_CASES (already lowered by build() for tests/test_gpu_fuzz.py) whose build gets a
# lane kernel, as (seed, build): read off the cross-compile reports, asserted by tests/test_lane_walk_cpu.py
FUZZ_LANE = [(0, "fast"), (0, "strict"), (2, "fast"), (2, "strict"), (3, "fast"), (4, "fast"), (4, "strict"), (5, "fast"), (5, "strict"),
             (6, "fast"), (7, "strict"), (8, "fast"), (9, "fast"), (10, "fast"), (11, "fast")]


def fuzz_spec(seed, kw, npoints=0):
    return gpu_fuzz_case("slots", seed, dict(kw, npoints=npoints))


def build_cases():
    """what build() lowers for the cases above, as (name, spec, opts keywords): every case at its small build size"""
    return [(c.name, c.make(c.n_build)[0], c.opts) for c in CASES]
