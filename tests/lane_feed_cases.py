"""The models the row feed of the lane walk (csrc/device/rh_lane.hip.h: rh_grad_lane_kernel, in a code object of its own, with
the rows taken from an interleaved copy of a target's columns, one set of rows requested ahead) is tested on, shared by the
cross-compile checks (tests/test_lane_feed_cpu.py), the device tests (tests/test_gpu_lane_feed.py) and build() (__graft_entry__.py
build_jobs, so that the device tests compile nothing).  No device is needed here.

linreg with k covariates has one row target of NC = k + 1 columns (y and the covariates); fit_normal has one column, wide8 eight.
A case is (model, build) with what the
cross-compile report says of it: `cols` -- the model has the column-fed kernel at all --, `rows` -- it has the row-fed one --,
`why` -- a piece of the reason where an eligible target's kernel was built and dropped.  Read off the reports;
tests/test_lane_feed_cpu.py holds every line to them."""
import numpy as np

from rainier_amd import _capi, models
from rainier_amd.frontend import Graph

FAST = dict(fp_contract=True, factor_outputs=True)
STRICT = dict(math_mode=_capi.MATH_STRICT)
BUILDS = {"fast": FAST, "strict": STRICT}

LANE = "rh_grad_lane_kernel"      # the entry point of either feed, each in a code object of its own (report tags "lane", "lane_rows")

# the row counts of the bit-identity tests, with gradSplits 8 (a block is 8 rows -- 4 in the strict build of k = 3 --, a split is
# ceil(blocks / 8) blocks, a wavefront's piece ceil(that / 8) blocks, a set 8 / 4 / 2 rows for NC <= 2 / 4 / 8):
#   1     one ragged row in the first piece of the first split, every other piece and split empty
#   9     one block = one piece of exactly one set (two sets for NC 4), and a single row in the second split
#   515   65 blocks, 9 per split, 2 per piece: four pieces of two blocks, one of one block (for NC <= 2 a single set: no pair), three
#         empty; the rows run out in the eighth split, which is one block and three single rows.  With blocks of 4 rows: pieces of
#         3 sets, an odd count (the last set is requested by the pair before it)
#   4099  513 blocks, 65 per split, 9 per piece: nine sets for NC <= 2, odd again; the eighth wavefront's piece is shorter than the
#         others; the last split ends in three blocks and three single rows, its eighth piece is empty
ROW_COUNTS = (1, 9, 515, 4099)
SPLITS = 8
N_MAIN = 4099
N_BUILD = 9          # what build() lowers (the generated source does not depend on the row count)
CHAINS, ITERATIONS, L = 130, 6, 4      # a full chain group and a ragged one of two chains


def wide8(n, seed=41):
    """a regression on two sums of covariates, so that the row has 8 columns and few sums: theta = (s, a, b), linreg's prior,
    y | x ~ N(a (x1 + x3 + x5 + x7) + b (x2 + x4 + x6), e^s) over n rows of (y, x1 .. x7)"""
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal(n) for _ in range(7)]
    y = 0.3 + 0.5 * sum(xs[0::2]) - 0.25 * sum(xs[1::2]) + 0.6 * rng.standard_normal(n)
    g = Graph(3, [0, 8])
    s, a, b = g.param(0), g.param(1), g.param(2)
    prior = (s - s.exp()) + models.std_normal_logpdf(a) + models.std_normal_logpdf(b)
    r = g.col(1, 0) - (a * (g.col(1, 1) + g.col(1, 3) + g.col(1, 5) + g.col(1, 7)) + b * (g.col(1, 2) + g.col(1, 4) + g.col(1, 6)))
    t = r * r * (s * -2.0).exp() / -2.0 - s
    return models.ModelSpec("wide8_%d" % n, g.compile([prior, t]), [y] + xs, [0, n], 3, {"kind": "wide8"})


def fit_normal(n):
    return models.fit_normal(np.random.default_rng(33).normal(1.5, 0.8, size=n))


class Case:
    def __init__(self, name, make, nc, build, cols, rows, why=None):
        self.make, self.nc, self.build, self.opts, self.cols, self.rows, self.why = make, nc, build, BUILDS[build], cols, rows, why
        self.name = "%s-%s" % (name, build)

    def __repr__(self):
        return self.name


def _linreg(k, *a, **kw):
    return Case("linreg%d" % k, lambda n: models.linreg(n=n, k=k), k + 1, *a, **kw)


CASES = [
    _linreg(3, "fast", True, True),        # cfg 2, the bench build: NC 4, sets of 4 rows
    _linreg(3, "strict", True, True),      # blocks of 4 rows (the column feed's 8 spill scalar registers): a set is a block
    _linreg(1, "fast", True, True),        # NC 2: sets of 8 rows
    _linreg(1, "strict", True, False, "eight wavefronts per SIMD would be lost"),    # 74 vector registers against the column feed's 62
    Case("fit_normal", fit_normal, 1, "fast", True, True),       # NC 1: a set is one 64-byte request
    Case("fit_normal", fit_normal, 1, "strict", True, True),
    Case("wide8", wide8, 8, "fast", True, True),                 # NC 8: blocks of 4 rows, sets of 2
    Case("wide8", wide8, 8, "strict", False, False),             # (no lane walk in the strict build)
    _linreg(7, "fast", False, False),      # NC 8 -- but 9 sums per chain: 72 KB of LDS, no lane walk at all
    _linreg(7, "strict", False, False),
    _linreg(2, "fast", True, False),       # NC 3: rows of 24 bytes do not tile a 64-byte line; the column feed stays
    _linreg(2, "strict", True, False),
]
BY_NAME = {c.name: c for c in CASES}
ROW_FED = [c for c in CASES if c.rows]
OTHER_WIDTHS = [c for c in ROW_FED if not c.name.startswith("linreg3")]      # NC 2, 1, 1 and 8


def build_cases():
    """what build() lowers for the cases above, as (name, spec, opts keywords)"""
    return [(c.name, c.make(N_BUILD), c.opts) for c in CASES]
