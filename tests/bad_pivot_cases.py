"""Cases of tests/test_gpu_bad_pivot.py (the device) and tests/test_bad_pivot_host.py (their proof against LAPACK), in one place
so that the two cannot drift apart: the problems, the two constructions of a covariance whose first non-positive pivot is known
without the device, and a model of the factorisation's schedule that turns a size and the handle's option values into the rows
where a failure is planted.  No GPU and no library call in here.

Construction (a), `planted_diag`: a per-point diagonal v (mi_gp_set_diag) that is zero except v[p] = -2 (kd + gv + jitter).  The
leading p x p block of K + (gv + jitter) I + diag(v) is the good problem's, so pivots 1 .. p are its pivots (positive: the good
problem factorises); pivot p + 1 is K_pp + gv + jitter + v_p minus a sum of squares <= -(kd + gv + jitter) < 0.  The index p + 1
is exact in real arithmetic with a margin of kd (no rounding decides it), for every kernel, theta, size and p.

Construction (b), `repeated_point_problem`: X[p] = X[q] for one q < p, gv = 0 and jitter = -0.05 kv at a short length scale.  Rows
p and q of K are equal, so the Schur complement of pivot p + 1 is at most (kv + jitter) - (kv + jitter) = 0 before the other
columns take their squares, and jitter < 0 pushes it to about 2 jitter; the leading block stays positive definite as long as the
length scale keeps K near kv I.  These are conditions on the INPUTS that test_bad_pivot_host.py checks with dpotrf for every
case below: every earlier pivot >= 1e-3 kv, the failing Schur complement <= -1e-3 kv."""
import numpy as np

KERNEL = "Matern52"
KERNS, OPS = ["Matern52"], []
D = 4

# ------------------------------------------------------------------------------------------------- the schedule, as a model
# Thresholds of csrc/gp_sched.hip that are NOT options (include/mi_gp.h states them in the text of options 0, 4-6, 30, 35 and 37):
LOOKAHEAD_MIN_TILES = 20      # two streams with look-ahead from this many tile columns on (option 0 = 1)
COLUMN_MODE_MIN_TILES = 4     # ... and from this many on when the whole problem runs in column mode
NARROW_PANELS_MAX_TILES = 60  # with look-ahead active, problems of up to this many tile columns use super-panels of at most 4 tiles
EXT_MIN_REST = 8              # no extended super-panel in front of the last this-many tile columns
U_EARLY_MIN_TILES = 64        # option 30: gradient evaluations from this many tile columns on
# the options the model reads (mi_gp_get_option), with the defaults of mi_gp_create for the modules that have no handle
SCHEDULE_OPTIONS = (0, 2, 4, 5, 6, 20, 21, 30, 35, 37, 46)
DEFAULT_OPTIONS = {0: 1, 2: 0, 4: 1 << 20, 5: 0, 6: 0, 20: 72, 21: 8, 30: 16, 35: 32, 37: 24, 46: 31}


def schedule(ntc, o):
    """What cholesky_enqueue (csrc/gp_sched.hip) does with one evaluation of `ntc` tile columns under the option values `o`:
    {"two": two streams, "panels": [(first tile column, width, extended, its update rides in the bulk update)], "tail": first tile
    column of column mode (None: no column mode), "early": option 30's early start of U = L^-T in a gradient evaluation}."""
    whole = o[37] > 0 and (ntc <= o[37] or ntc <= o[46])
    two = o[0] == 2 or (o[0] == 1 and ntc >= (COLUMN_MODE_MIN_TILES if whole else LOOKAHEAD_MIN_TILES))
    cap = 4 if (two and ntc <= NARROW_PANELS_MAX_TILES) else 0

    def pick_w(rem):
        w = o[2]
        if w <= 0:
            w = 16 if rem > o[4] else 8 if rem > o[5] else 4 if rem > o[6] else 2
            if cap and w > cap:
                w = cap
        return min(rem, w)

    def column_mode(c0):
        return o[37] > 0 and c0 < ntc and (ntc - c0 <= o[37] or (c0 == 0 and whole))

    def extended(c0, w):
        return o[35] > 0 and ntc >= LOOKAHEAD_MIN_TILES and (ntc + 1) - (c0 + w) <= o[35] and ntc - (c0 + w) > EXT_MIN_REST

    out = {"two": two, "panels": [], "tail": None, "early": two and o[30] > 0 and ntc >= U_EARLY_MIN_TILES}
    if column_mode(0):
        out["tail"] = 0
        return out
    c0, on_two, prev_ext = 0, two, False
    while c0 < ntc:
        w = pick_w(ntc - c0)
        if c0 > 0 and on_two and ntc - c0 <= o[21]:
            on_two = False  # (option 21: the rest on the main stream alone)
        rides = c0 > 0 and on_two and c0 + w < ntc and not prev_ext and o[20] > 0 and ntc - c0 >= o[20]
        ext = extended(c0, w)
        out["panels"].append((c0, w, ext, rides))
        prev_ext = ext
        c0 += w
        if column_mode(c0):
            out["tail"] = c0
            break
    return out


def positions(n, o):
    """{name: 0-based row p of the failing pivot} for a problem of n points under the option values `o`.  A position that does
    not exist at this size is left out by the rule written at its line; two names for the same row keep the first."""
    ntc = (n + 127) // 128
    s = schedule(ntc, o)
    want = []
    # leaf block and tile edges: the 16-pivot ballot of the leaf (rows 0, 15 | 16) and its two-pivot form; the first tile's
    # last row and the second tile's first
    for r in (0, 1, 15, 16, 127, 128):
        want.append((f"row{r}", r))  # (left out where r >= n, below)
    pan = s["panels"]
    if pan:  # super-panels exist (not a problem that runs in column mode from its first column)
        c0, w, _, _ = pan[0]
        want.append(("panel1_middle", (c0 * 128 + (c0 + w) * 128) // 2))
        want.append(("panel1_last_col", (c0 + w) * 128 - 1))
    if len(pan) >= 2:  # a second super-panel: factored beside the first bulk update when two streams run
        c0, w, _, _ = pan[1]
        want.append(("panel2_first_col", c0 * 128))
        want.append(("panel2_last_col", (c0 + w) * 128 - 1))
    rides = [q for q in pan if q[3]]
    if rides:  # a super-panel whose update rode at the head of the bulk update (option 20)
        c0, w, _, _ = rides[0]
        want.append(("riding_panel_first_col", c0 * 128))
        want.append(("riding_panel_last_col", (c0 + w) * 128 - 1))
    exts = [q for q in pan if q[2]]
    if exts:  # an extended super-panel (option 35), and the column behind it that its in-panel updates also wrote
        c0, w, _, _ = exts[0]
        want.append(("extended_panel_first_col", c0 * 128))
        want.append(("extended_panel_last_col", (c0 + w) * 128 - 1))
        want.append(("behind_extended_panel", (c0 + w) * 128 + 17))
    if s["tail"] is not None and ntc - s["tail"] >= 2:  # column mode over at least two columns
        t = s["tail"]
        want.append(("tail_first_col", t * 128))
        want.append(("tail_middle", ((t + ntc) // 2) * 128 + 64))
    want.append(("last_col_first_pivot", (ntc - 1) * 128))
    want.append(("last_row", n - 1))
    out, seen = {}, set()
    for name, p in want:
        if 0 <= p < n and p not in seen:
            out[name] = p
            seen.add(p)
    return out


# ------------------------------------------------------------------------------------------------- construction (a)
# N of the single-handle cases by what the schedule does with them at today's defaults (the GPU module recomputes everything
# from the handle's options and asserts that every schedule of the list is hit):
#   one stream, column mode: 1, 3 tile columns | two streams, column mode from the start: 4, 7, 8, 19, 24, 31 | the turn at
#   option 46: 32, 33 | panels + look-ahead + extended super-panels + column-mode tail: 32, 33, 40, 52 | option 30: 66, 81 |
#   riding update (80 tile columns and more): 81.   N % 128 != 0 in 10 of the 14.
SINGLE_SIZES = (100, 384, 500, 896, 1000, 2400, 3072, 3900, 4096, 4150, 5100, 6600, 8400, 10300)
HOST_NUMERIC_MAX_N = 2400  # test_bad_pivot_host.py runs dpotrf on every position up to this size; above it the argument holds


def problem(n):
    from oracle import gp_oracle as orc

    return orc.synth_problem(n, D, seed=n)


def good_theta(which=0):
    """Two ordinary hyper-parameter vectors (every field differs between them)."""
    from oracle import gp_oracle as orc

    th = orc.synth_theta(D)
    if which:
        th[:D] *= np.array([0.8, 1.3, 0.9, 1.15])
        th[D] = 1.1
        th[-2], th[-1] = 3e-4, 2e-6
    return th


def prior_variance(theta):
    return float(theta[D])  # one component: kd = kv


def planted_diag(n, p, theta):
    v = np.zeros(n)
    v[p] = -2.0 * (prior_variance(theta) + theta[-2] + theta[-1])
    return v


# ------------------------------------------------------------------------------------------------- construction (b)
BAD_KV = 1.7


def bad_ls(n):
    """Short enough that the leading block stays positive definite at n Latin-hypercube points in [0, 1]^4 (at 0.05 the data of
    4150 points are indefinite from pivot 3451 on, at 0.03 those of 6200 from 2882 on: the host module measures the room)."""
    return 0.05 if n <= 1500 else 0.03 if n <= 4150 else 0.02


def bad_theta(n, kv=BAD_KV):
    """ls = bad_ls(n), gv = 0, jitter = -0.05 kv.  K + jitter I = kv (C - 0.05 I) with C the correlation matrix: kv scales every pivot, so the
    index does not depend on it (and a power-of-two factor leaves dpotrf's decisions bit for bit the same)."""
    from oracle import gp_oracle as orc

    return orc.pack_theta(np.full((1, D), bad_ls(n)), [kv], 0.0, -0.05 * kv)


def minus_ten_theta():
    """jitter = -10 on an ordinary theta: kd + gv + jitter < 0, the first pivot fails (index 1)."""
    th = good_theta(0)
    th[-1] = -10.0
    return th


def repeated_point_problem(n, p, q):
    """synth_problem(n) with X[p] = X[q], q < p."""
    X, y = problem(n)
    assert 0 <= q < p < n
    X = X.copy()
    X[p] = X[q]
    return X, y


# batches of K = 5 on one data set per size: (n, p, q) -- 3, 8, 24, 33 and 49 tile columns, the failure deep in each
BATCH_CASES = ((300, 290, 213), (1000, 900, 823), (3000, 2700, 2623), (4150, 4100, 4023), (6200, 5000, 4923))
# sharded driver on one rank: (n, panel width in tiles, p, q) -- 3 panels (12 tile columns) and 9 panels (33 tile columns); p in
# the first panel, in the first column of a later panel, in the last panel
DIST_CASES = ((1500, 4, 300, 223), (1500, 4, 512, 435), (1500, 4, 1203, 1126),
              (4150, 4, 400, 323), (4150, 4, 2048, 1971), (4150, 4, 4120, 4043))


def repeated_point_cases():
    """Every (n, p, q) of construction (b), for the host proof."""
    return sorted(set(BATCH_CASES) | {(n, p, q) for n, _, p, q in DIST_CASES})
