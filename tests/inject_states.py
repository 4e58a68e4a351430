"""Injected ninja states for the step kernel: (level, x, y, vx, vy, family) rows plus per-tick input bytes for TICKS ticks,
deterministic and seeded (tests/test_inject_host.py, tests/test_gpu_inject.py, tests/golden/make_golden_inject.py; DESIGN.md
"injected states").  A rollout from the spawn point only ever perturbs the previous tick; these rows put position and velocity
where no rollout gets: inside solids, at speeds the ninja's own physics cannot reach, on the 12 px lattice to the ulp.

Every simulator is reset, gets row k written over xpos, ypos, xspeed, yspeed (Oracle.set_ninja, NppBatch.set_ninja_state, plain
attribute assignment in the reference) and then runs TICKS ticks under inputs()[:, k].

Levels: the curriculum-0 levels 84 (quarter circles all around), 14 (straight segments only), 29 (the V crease), and one
synthetic map (synthetic_map) that shows every tile id 1..33 once with empty cells all around it, a flat floor of full tiles over
x in [24, 120] whose top is y = FLOOR_TOP, and no entity but spawn, exit door and exit switch.

Families:
  free      position uniform over [24, 1032] x [24, 576] -- inside solids as often as the level is solid --, v ~ N(0, 3)
  fast      same positions, v ~ N(0, 12) (FAST12) or N(0, 45) (FAST45), |v| scaled down to 200: sweeps over many cells (more than
            three columns from |vx| > 26 on, where the candidate registers give way to the table walk), time of impact against
            every shape from every side
  lattice   x = 12 i + o, y = 12 j + o' with o, o' from LATTICE_OFFSETS: contact and exit thresholds (10 and 10 -+ 1e-7), the wall
            probe's radius 10.1 and its |dy| < 1e-5 gate (1e-8), cell bounds x = 24 k exactly, query boxes that touch a cell
            bound.  Three groups in four stand next to the level's geometry (an end point of a table segment, -1..1 lattice steps
            away), the fourth anywhere.  Rows come in groups of 5 ulp-neighbours (k = -2..2 ulp on x, on y, or on both; `group`
            numbers them); v is 0 or N(0, 0.5), one draw per group.  The tick integrates before it collides, so with v = 0 the
            x thresholds meet the collision code exactly and the y ones moved by one step of gravity
  bandaid   on the synthetic floor: x is each of the reference's three hard-coded positions (ninja.py:315-318) and its two
            neighbouring doubles, y puts the ninja 0.5 px into the floor, v = 0, so the closest point lies straight below and
            abs(dx) <= 1e-7 holds by construction
  corners   synthetic level: around every point where two segments of the compiled table meet (of the border's vertices only those
            around the map's top-left corner: the rest repeat them), vertex + r (cos, sin) for 16 angles
            and r in CORNER_RADII: first-wins ties between the two, front / back bias flips.  v is 0 (even vertex) or N(0, 0.5)
"""
import functools

import numpy as np

TICKS = 6
SEED = 20241
LEVEL_IDS = (84, 14, 29, -1)   # index into curriculum0_levels(); -1: the synthetic map
ARCS, STRAIGHT, CREASE, SYNTH = 0, 1, 2, 3   # the `level` column: an index into LEVEL_IDS / level_maps()
FREE, FAST12, FAST45, LATTICE, BANDAID, CORNERS = 0, 1, 2, 3, 4, 5
FAMILY_NAMES = ("free", "fast12", "fast45", "lattice", "bandaid", "corners")
N_FREE, N_FAST12, N_FAST45, N_LATTICE_GROUPS = 1500, 750, 750, 500   # per level
BANDAID_X = (50.51197510492316, 49.23232124849253, 49.153536108584795)
LATTICE_OFFSETS = (0.0, 10.0, -10.0, 10.1, -10.1, 10.0 - 1e-7, -(10.0 - 1e-7), 10.0 + 1e-7, -(10.0 + 1e-7), 1e-8, -1e-8)
CORNER_RADII = (5.0, 9.999, 10.0, 10.0999)
V_MAX = 200.0
FLOOR_ROW = 11                   # cell row of the synthetic floor (cells 1..4 of that row are full tiles)
FLOOR_TOP = 24.0 * FLOOR_ROW
EXHIBIT_ROWS, EXHIBIT_COL0 = (3, 5), 7   # cell rows of the exhibited tiles; they stand in every second column from EXHIBIT_COL0 on


def exhibit_cells():
    """{tile id: (cell x, cell y)} of the synthetic map, ids 1..33 (id 0 is every other cell: it has no segment)."""
    out = {}
    for t in range(1, 34):
        k = t - 1
        out[t] = (EXHIBIT_COL0 + 2 * (k % 17), EXHIBIT_ROWS[k // 17])
    return out


def synthetic_map():
    """f64 map_data blob (the layout of the curriculum-0 blobs: tiles at 184 + x + 42 y, exit door count at 1156, then the
    5-value records spawn, exit door, exit switch in units of 6 px from 1230 on)."""
    m = np.zeros(1245, dtype=np.float64)
    tiles = np.zeros((23, 42), dtype=np.float64)   # [y, x] of the inner area; cell (cx, cy) is tiles[cy - 1, cx - 1]
    for t, (cx, cy) in exhibit_cells().items():
        tiles[cy - 1, cx - 1] = t
    tiles[FLOOR_ROW - 1, 0:4] = 1
    m[184:184 + 42 * 23] = tiles.ravel()
    m[1156] = 1
    m[1230:1245] = [0, 84, 66, 1, 0, 3, 120, 80, 0, 0, 4, 140, 80, 0, 0]   # spawn (504, 396), door (720, 480), switch (840, 480)
    return m


@functools.lru_cache(maxsize=None)
def level_maps():
    """The four map blobs in `level` column order."""
    from nclone_amd.levels import curriculum0_levels

    c0 = curriculum0_levels()[0]
    out = tuple(np.asarray(c0[i], dtype=np.float64) if i >= 0 else synthetic_map() for i in LEVEL_IDS)
    for m in out:
        m.setflags(write=False)
    return out


def tile_grid(m):
    """[44, 25] tile ids of a blob incl. the solid border (the layout of Oracle.tiles)."""
    t = np.ones((44, 25), dtype=np.int64)
    t[1:43, 1:24] = np.asarray(m[184:184 + 42 * 23]).reshape(23, 42).T
    return t


def ulp_shift(v, k):
    """v moved k doubles up (k > 0) or down."""
    v = np.array(v, dtype=np.float64)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return v


def segment_vertices(rows):
    """Points shared by two or more segments of a compiled table (rows of compile_level_segments): sorted unique (x, y)
    int array.  A linear row's ends are (x1, y1), (x2, y2); an arc row's are (cx + 24 hor, cy) and (cx, cy + 24 ver)."""
    r = rows.astype(np.int64)
    lin = r[:, 2] == 0
    a = np.where(lin[:, None], r[:, 3:5], np.stack([r[:, 3] + 24 * r[:, 5], r[:, 4]], axis=1))
    b = np.where(lin[:, None], r[:, 5:7], np.stack([r[:, 3], r[:, 4] + 24 * r[:, 6]], axis=1))
    pts, cnt = np.unique(np.concatenate([a, b]), axis=0, return_counts=True)
    return pts[cnt >= 2]


def _clip_speed(v):
    n = np.sqrt((v * v).sum(axis=1))
    return v * np.minimum(1.0, V_MAX / np.maximum(n, 1e-300))[:, None]


def _uniform_family(rng, n, sigma):
    x = rng.uniform(24.0, 1032.0, n)
    y = rng.uniform(24.0, 576.0, n)
    v = _clip_speed(rng.normal(0.0, sigma, (n, 2)))
    return np.column_stack([x, y, v])


def _lattice_family(rng, n_groups, level):
    from nclone_amd.engine import compile_level_segments

    i = rng.integers(2, 87, n_groups)
    j = rng.integers(2, 49, n_groups)
    # three groups in four stand at a lattice point next to the level's geometry: an end point of a random row of the compiled
    # segment table (every tile coordinate is a multiple of 12), moved by -1..1 lattice steps each way
    seg = compile_level_segments(level_maps()[level])[0].astype(np.int64)
    seg = seg[(seg[:, 2] == 0) & (seg[:, 0] >= 1) & (seg[:, 0] <= 42) & (seg[:, 1] >= 1) & (seg[:, 1] <= 23)]
    pick = seg[rng.integers(0, len(seg), n_groups)]
    end = rng.integers(0, 2, n_groups)
    step = np.array([-1, 0, 0, 1])
    ai = np.where(end == 0, pick[:, 3], pick[:, 5]) // 12 + step[rng.integers(0, 4, n_groups)]
    aj = np.where(end == 0, pick[:, 4], pick[:, 6]) // 12 + step[rng.integers(0, 4, n_groups)]
    anchored = np.arange(n_groups) % 4 != 0
    i = np.where(anchored, np.clip(ai, 2, 86), i)
    j = np.where(anchored, np.clip(aj, 2, 48), j)
    off = np.array(LATTICE_OFFSETS)
    x = 12.0 * i + off[rng.integers(0, len(off), n_groups)]
    y = 12.0 * j + off[rng.integers(0, len(off), n_groups)]
    v = rng.normal(0.0, 0.5, (n_groups, 2)) * (np.arange(n_groups) % 2)[:, None]
    rows = []
    for g in range(n_groups):
        mode = (g // 2) % 3   # which coordinate walks through its ulp-neighbours: x, y, both
        for k in range(-2, 3):
            rows.append([ulp_shift(x[g], k) if mode != 1 else x[g], ulp_shift(y[g], k) if mode != 0 else y[g], v[g, 0], v[g, 1]])
    return np.array(rows, dtype=np.float64), np.repeat(np.arange(n_groups), 5)


def _bandaid_family():
    rows = []
    for x in BANDAID_X:
        for k in (-1, 0, 1):
            rows.append([ulp_shift(x, k), FLOOR_TOP - 10.0 + 0.5, 0.0, 0.0])
    return np.array(rows, dtype=np.float64)


def _corner_family(rng):
    from nclone_amd.engine import compile_level_segments

    seg, _ = compile_level_segments(level_maps()[SYNTH])
    pts = segment_vertices(seg).astype(np.float64)
    # the border's own vertices (about 600) all repeat one straight continuation of two collinear segments: the ones around the
    # map's top-left inner corner stand for them
    inside = (pts[:, 0] > 24) & (pts[:, 0] < 1032) & (pts[:, 1] > 24) & (pts[:, 1] < 576)
    pts = pts[inside | ((pts[:, 0] <= 72) & (pts[:, 1] <= 72))]
    ang = 2.0 * np.pi * np.arange(16) / 16.0
    rows = []
    for n, (px, py) in enumerate(pts):
        v = rng.normal(0.0, 0.5, 2) * (n % 2)
        for r in CORNER_RADII:
            for a in ang:
                rows.append([px + r * np.cos(a), py + r * np.sin(a), v[0], v[1]])
    return np.array(rows, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def states():
    """(level i32 [n], xyv f64 [n, 4], family i32 [n], group i32 [n]): rows ordered by level, inside a level by family; `group`
    numbers the ulp-neighbour groups of the lattice family (unique across levels) and is -1 elsewhere.  Read-only arrays."""
    rng = np.random.default_rng(SEED)
    lv, xyv, fam, grp = [], [], [], []
    n_groups = 0

    def add(level, family, rows, groups=None):
        nonlocal n_groups
        lv.append(np.full(len(rows), level, dtype=np.int32))
        xyv.append(rows)
        fam.append(np.full(len(rows), family, dtype=np.int32))
        if groups is None:
            grp.append(np.full(len(rows), -1, dtype=np.int32))
        else:
            grp.append((groups + n_groups).astype(np.int32))
            n_groups += int(groups.max()) + 1

    for level in range(len(LEVEL_IDS)):
        add(level, FREE, _uniform_family(rng, N_FREE, 3.0))
        add(level, FAST12, _uniform_family(rng, N_FAST12, 12.0))
        add(level, FAST45, _uniform_family(rng, N_FAST45, 45.0))
        add(level, LATTICE, *_lattice_family(rng, N_LATTICE_GROUPS, level))
        if level == SYNTH:
            add(level, BANDAID, _bandaid_family())
            add(level, CORNERS, _corner_family(rng))
    out = (np.concatenate(lv), np.concatenate(xyv), np.concatenate(fam), np.concatenate(grp))
    assert np.isfinite(out[1]).all()
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def inputs():
    """uint8 [TICKS, n] replay input bytes (bit 0 jump, bit 1 right, bit 2 left), one seeded random byte per state and tick."""
    n = len(states()[0])
    a = np.random.default_rng(SEED + 1).integers(0, 8, size=(TICKS, n)).astype(np.uint8)
    a.setflags(write=False)
    return a


_ORACLE = {}


def oracle_run(om, variant):
    """The oracle's run of every row (om: the oracle module, variant "pow" or "mul"): (F f64 [n, TICKS, 12], D i32 [n, TICKS, 22],
    valid bool [n, TICKS]).  valid[k, t]: no earlier tick left row k terminal (state 6, 7 or 8), i.e. tick t is compared.
    Computed once per variant, shared by the tests, read-only."""
    if variant not in _ORACLE:
        level, xyv, _, _ = states()
        inp = inputs()
        n = len(level)
        F = np.zeros((n, TICKS, 12), dtype=np.float64)
        D = np.zeros((n, TICKS, 22), dtype=np.int32)
        hor_jump = [om.controls(b) for b in range(8)]
        for lv, m in enumerate(level_maps()):
            o = om.Oracle(variant)
            o.load(m)
            for k in np.nonzero(level == lv)[0]:
                o.reset()
                o.set_ninja(*xyv[k])
                for t in range(TICKS):
                    o.tick(*hor_jump[inp[t, k]])
                    f, d = o.core()
                    F[k, t], D[k, t] = f, d[:22]
        terminal = np.isin(D[:, :, 0], (6, 7, 8))
        valid = np.ones((n, TICKS), dtype=bool)
        valid[:, 1:] = ~(np.cumsum(terminal, axis=1)[:, :-1] > 0)
        for a in (F, D, valid):
            a.setflags(write=False)
        _ORACLE[variant] = (F, D, valid)
    return _ORACLE[variant]


def golden_subset():
    """Indices into states() of the rows the reference fixture tests/golden/inject.npz holds: every bandaid row and every
    `stride`-th row of each (level, family), whole ulp-neighbour groups for the lattice family -- chosen by position in the
    table alone."""
    level, _, family, group = states()
    pick = []
    for lv in range(len(LEVEL_IDS)):
        for f, stride in ((FREE, 5), (FAST12, 5), (FAST45, 3), (LATTICE, 4), (BANDAID, 1), (CORNERS, 16)):
            idx = np.nonzero((level == lv) & (family == f))[0]
            if f == LATTICE:
                idx = idx[(group[idx] - group[idx].min()) % stride == 0]
            else:
                idx = idx[::stride]
            pick.append(idx)
    return np.concatenate(pick)
