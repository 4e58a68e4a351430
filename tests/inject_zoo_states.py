"""Injected ninja AND mover states at the entity code's thresholds: the companion of tests/inject_states.py for the entity zoo
(tests/test_inject_zoo_host.py, tests/test_gpu_inject_zoo.py, tests/golden/make_golden_inject_zoo.py).  A rollout
meets an entity at whatever distance its physics produces; these rows put the ninja on the radii, square sides, planes and cell
bounds the entity code compares against, to the ulp, and put the movers where their own physics never takes them.

Every simulator gets row k's level, is reset (`fresh` rows are NOT: they run in the first creation of the entities, where death
balls repel each other), gets x, y, vx, vy written over the ninja (Oracle.set_ninja, NppBatch.set_ninja_state, attribute
assignment in the reference), gets up to two movers overwritten (Oracle.set_mover, NppBatch.set_mover_state: x, y, a, b and
optionally the thwump state / drone dir; attribute assignment in the reference) and runs TICKS ticks under inputs()[:, k].

Levels: all share the tiles, spawn (504, 396) and floor of inject_states.synthetic_map(); entity records are appended in the layout
tests/fuzz_levels.py documents, one per SLOT cell -- slots are 4 cells apart, so the 3 x 3 cell neighbourhoods of two entities
never touch each other, the spawn's or the exit pair's.
  PLAIN   toggle mines in both initial states (type 1: toggled, deadly; type 21: untoggled), gold, a locked door with its switch;
          the exit switch stands one cell left of the exit door (the door joins the grid only when its switch is hit: a row that
          touches both can test the door's radius at the second tick).  Selects the plain kernels.
  STATIC  regular door, trap door with its switch, launch pads and one-way platforms in all 8 orientations, two boost pads 12 px
          apart (touched in the same tick: the creation-order loop of zoo_think_static)
  MOVERS  zap drone, bounce block, thwumps in 4 orientations, death ball, mini drone, shove thwump
  BALLS   two death balls
  REAL    a recorded level with death balls next to tiles (zoo_levels())

A tick moves the entities and runs their think() BEFORE the ninja integrates (nsim.py:235-251), then the ninja integrates (drag,
gravity, position += speed; ninja.py:198-206) and only then collides.  So a threshold of move() / think() (boost pads, the mines'
3.5 / 4.5 radii, the thwump's line of sight, the death ball's chase) is met by the INJECTED position, and a threshold of a physical
or logical collision by the position AFTER the first integration.  Rows of the second sort are built backwards: the wanted
collision position P and speed come first, the injected position is P minus the integrated speed (a plain v = 0 row would miss
every radius by gravity's 0.0667 px: 1.4e-4 px on a 16 px radius, a thousand times the 1e-7 the thresholds are probed at).

Ninja families (`group` numbers ulp-neighbour groups: 5 rows that differ by -2..2 ulp in one coordinate):
  ring      centre + (R + d)(cos a, sin a), 16 angles, d in RING_D, R each radius the kind compares against (THRESHOLDS)
  square    bounce block / thwump / shove thwump: each side at semi-side + d for the physical and the logical semi-side, the
            diagonals (peny <= penx ties), the ends of the thwump's kill strip along its charging face, and the shove thwump's
            launch gate len2 > 0.2.  (Its other gate, xdir * depen_x + ydir * depen_y >= 0.01, is a product of axis-aligned unit
            vectors: it only takes the values -1, 0 and 1 and has no threshold to stand on.)
  oneway    per orientation: lateral +-17.1, +-21.1, normal 0 and 10, normal_dist_old 8.9, both signs of normal_proj / direction
  pad       launch pads: the -0.1 plane (normal distance 10.1) inside the 16 px ring; boost pads: speed exactly 0 between both
  lane      thwump's line of sight: across-axis distance 38 +- d, along-axis position through the cell bound at its face
  free, fast   uniform positions, v ~ N(0, 3) / N(0, 45) clipped to 200, on every level
Mover families (the ninja rests at the spawn unless noted):
  ball_free, ball_fast   the ball anywhere on the map (inside solids too), v ~ N(0, 1) / N(0, 20) clipped to 60
  ball_lattice  the ball on the 12 px lattice next to segment end points, offsets BALL_OFFSETS, ulp groups, exactly on segments too
  ball_speed    |v| after the chase term at 0.85, 0.85 + 0.01 / 0.9, 1.35 and the speed the clamp maps to 1.35, into the floor
  ball_pair     BALLS, fresh: ball 1 at 16 +- d from where ball 0 stands after its move
  thwump    retreating within a step of its origin; face within a step of a 12 px bound (free / blocked); crushing the ninja
            against the floor and the left wall at gaps around the ninja's 20 px
  drone     within 1e-6 / one step of its target, before and past it, every dir, both kinds
  bounce    the block displaced up to 40 px with v ~ N(0, 3), the ninja at `square` positions of where it moves to
A ninja exactly on a ball's centre is excluded by construction (no ring has radius 0; the reference divides by that distance).
"""
import functools
import math

import numpy as np

from tests import inject_states as base

TICKS = base.TICKS
SEED = 20251
V_MAX = 200.0
PLAIN, STATIC, MOVERS, BALLS, REAL = 0, 1, 2, 3, 4
LEVEL_NAMES = ("plain", "static", "movers", "balls", "real")
FAMILY_NAMES = ("ring", "square", "oneway", "pad", "lane", "free", "fast", "ball_free", "ball_fast", "ball_lattice", "ball_speed",
                "ball_pair", "thwump", "drone", "bounce")
(RING, SQUARE, ONEWAY, PAD, LANE, FREE, FAST, BALL_FREE, BALL_FAST, BALL_LATTICE, BALL_SPEED, BALL_PAIR, THWUMP, DRONE,
 BOUNCE) = range(len(FAMILY_NAMES))
N_FREE, N_FAST, N_BALL_FREE, N_BALL_FAST, N_BALL_LATTICE_GROUPS, N_BOUNCE = 600, 400, 600, 400, 240, 60
RING_D = (0.0, 1e-7, -1e-7, 1e-9, -1e-9)
BALL_OFFSETS = (0.0, 8.0, -8.0, 8.0 - 1e-7, -(8.0 - 1e-7), 8.0 + 1e-7, -(8.0 + 1e-7), 4.0, -4.0, 5.0, -5.0)
KEEP = -2                      # mover field: leave state / dir alone (oracle.KEEP_FIELD)
SPAWN = (504.0, 396.0)
GRAVITY, DRAG = 0.06666666666666665, 0.9933221725495059   # the ninja's after a reset (ninja.py:198-202: falling, regular drag)
DIAG = math.sqrt(2) / 2
MOVER_TYPES = (14, 17, 20, 25, 26, 28)

# (name, reference line, tick whose outcome the threshold decides).  The values themselves: npp_zoo.hpp logical_collisions_zoo /
# mover_logical / zoo_think_static / thwump_think / oneway_depen / mover_physical and npp_kernels.hip's plain twins.
THRESHOLDS = (
    ("mine_toggle_13.5", "entity_toggle_mine.py:95-102 (RADII[1] 3.5 + 10, think)", 0),
    ("mine_untoggle_14.5", "entity_toggle_mine.py:107-114 (RADII[2] 4.5 + 10, think, at the second tick)", 1),
    ("mine_kill_14", "entity_toggle_mine.py:124-126 (RADII[0] 4 + 10)", 0),
    ("gold_16", "entity_gold.py:67-69 (6 + 10)", 0),
    ("exit_door_22", "entity_exit.py:71-73 (12 + 10, at the second tick: the switch is hit at the first)", 1),
    ("exit_switch_16", "entity_exit_switch.py:79-81 (6 + 10)", 0),
    ("locked_switch_15", "entity_door_locked.py:57-59 (5 + 10)", 0),
    ("regular_door_20", "entity_door_regular.py:59-61 (10 + 10)", 0),
    ("trap_switch_15", "entity_door_trap.py:63-65 (5 + 10)", 0),
    ("launch_16", "entity_launch_pad.py:86-88 (6 + 10)", 0),
    ("boost_16", "entity_boost_pad.py:52-54 (6 + 10, move)", 0),
    ("zap_17.5", "entity_drone_zap.py:61-63 (7.5 + 10)", 0),
    ("mini_14", "entity_mini_drone.py:64-66 (4 + 10)", 0),
    ("ball_15", "entity_death_ball.py:173-175 (5 + 10)", 0),
    ("bounce_19", "entity_bounce_block.py:130-131 (SEMI_SIDE 9 + 10, physical)", 0),
    ("bounce_19.1", "entity_bounce_block.py:150-155 (9 + 10 + 0.1, logical)", 0),
    ("thwump_19", "entity_thwump.py:211-212 (9 + 10, physical)", 0),
    ("thwump_19.1", "entity_thwump.py:221-226 (9 + 10 + 0.1, logical)", 0),
    ("shove_22", "entity_shove_thwump.py:161-166 (12 + 10, physical)", 0),
    ("shove_22.1", "entity_shove_thwump.py:178-183 (12 + 10 + 0.1, logical)", 0),
    ("square_diagonal", "physics.py:195 (peny <= penx)", 0),
    ("thwump_strip_12", "entity_thwump.py:239-240 (overlap_circle_vs_segment, 10 + 2)", 0),
    ("oneway_lateral_17.1", "entity_one_way_platform.py:90-91 (0.51 * 10 + 12)", 0),
    ("oneway_lateral_21.1", "entity_one_way_platform.py:90-91 (0.91 * 10 + 12)", 0),
    ("oneway_normal_0", "entity_one_way_platform.py:93 (0 < normal_dist)", 0),
    ("oneway_normal_10", "entity_one_way_platform.py:93 (normal_dist <= 10)", 0),
    ("oneway_old_8.9", "entity_one_way_platform.py:101 (10 - normal_dist_old <= 1.1)", 0),
    ("launch_plane_10.1", "entity_launch_pad.py:89-94 (>= -0.1)", 0),
    ("boost_speed_0", "entity_boost_pad.py:57 (vel_norm > 0)", 0),
    ("lane_38", "entity_thwump.py:162-165, 187 (2 * (9 + 10))", 0),
    ("lane_cell", "entity_thwump.py:166-171, 188 (ninja cell against the thwump's face cell)", 0),
    ("shove_launch_0.2", "entity_shove_thwump.py:189 (depen[1][1] > 0.2: the other axis' penetration of the logical square)", 0),
)
THR = {name: i for i, (name, _, _) in enumerate(THRESHOLDS)}
RING_RADII = {21: (("mine_toggle_13.5", 13.5, "pre"), ("mine_untoggle_14.5", 14.5, "leave")), 1: (("mine_kill_14", 14.0, "post"),),
              2: (("gold_16", 16.0, "post"),), 3: (("exit_door_22", 22.0, "rest2"),), 4: (("exit_switch_16", 16.0, "post"),),
              6: (("locked_switch_15", 15.0, "post"),), 5: (("regular_door_20", 20.0, "post"),), 8: (("trap_switch_15", 15.0, "post"),),
              10: (("launch_16", 16.0, "post"),), 24: (("boost_16", 16.0, "pre"),), 14: (("zap_17.5", 17.5, "post"),),
              26: (("mini_14", 14.0, "post"),), 25: (("ball_15", 15.0, "ball"),)}
SQUARE_SEMI = {17: ("bounce_19", 19.0, "bounce_19.1"), 20: ("thwump_19", 19.0, "thwump_19.1"), 28: ("shove_22", 22.0, "shove_22.1")}


def slots():
    """cells (cx, cy) entities may stand in: 4 apart, none within one cell of the spawn's, the exit door's or the exit switch's
    cell (either place of the switch), the exhibited tiles or the floor"""
    out = []
    for cy in (8, 12, 16, 20):
        for cx in range(7, 40, 4):
            if (cy == 16 and cx in (19, 23)) or (cy == 20 and cx in (27, 31, 35)):
                continue
            out.append((cx, cy))
    return out


def _u(cell, off=(2, 2)):
    """map units (6 px) of a point of a cell: off (2, 2) is its centre"""
    return 4 * cell[0] + off[0], 4 * cell[1] + off[1]


@functools.lru_cache(maxsize=None)
def level_specs():
    """per level: list of entity records (type, x, y, orientation, mode[, switch x, switch y]) in map units, in map order after
    the base map's spawn, exit door, exit switch"""
    s = slots()
    plain = [(1,) + _u(s[0]) + (0, 0), (21,) + _u(s[1]) + (0, 0), (2,) + _u(s[2]) + (0, 0),
             (6,) + _u(s[3]) + (0, 0) + _u(s[4])]
    static = [(5,) + _u(s[0]) + (0, 0), (8,) + _u(s[1]) + (2, 0) + _u(s[2])]
    static += [(10,) + _u(s[3 + o]) + (o, 0) for o in range(8)]
    static += [(11,) + _u(s[11 + o]) + (o, 0) for o in range(8)]
    static += [(24,) + _u(s[19], (1, 2)) + (0, 0), (24,) + _u(s[19], (3, 2)) + (0, 0)]
    movers = [(20,) + _u(s[9 + k]) + (o, 0) for k, o in enumerate((0, 2, 4, 6))]
    movers += [(28,) + _u(s[14]) + (0, 0), (17,) + _u(s[15]) + (0, 0), (14,) + _u(s[2]) + (0, 2), (26,) + _u(s[4]) + (2, 2),
               (25,) + _u(s[6]) + (0, 0)]
    balls = [(25,) + _u(s[12]) + (0, 0), (25,) + _u(s[13]) + (0, 0)]
    return plain, static, movers, balls


def _with_entities(m, spec):
    extra = []
    for e in spec:
        extra += list(e[:5]) + ([0, e[5], e[6], 0] if len(e) > 5 else [])
    out = np.concatenate([m, np.array(extra, dtype=np.float64)])
    out[1200] = sum(e[0] == 25 for e in spec)
    return out


def _real_level():
    """the first recorded zoo level with two or more death balls (map_data[1200]) and at most N_MOVERS_MAX movers -- balls among
    real tiles"""
    from nclone_amd.engine import compile_level_zoo
    from nclone_amd.levels import zoo_levels

    for m in zoo_levels()[0]:
        if len(m) > 1200 and m[1200] >= 2 and len(compile_level_zoo(m)[2]) <= N_MOVERS_MAX:
            return np.asarray(m, dtype=np.float64).copy()
    raise AssertionError("no recorded level with death balls")


@functools.lru_cache(maxsize=None)
def level_maps():
    """The five map blobs in `level` column order (read-only)."""
    out = []
    for lv, spec in enumerate(level_specs()):
        m = base.synthetic_map().copy()
        if lv == PLAIN:
            m[1240:1243] = [4, 116, 80]   # exit switch at (696, 480), 24 px left of the door at (720, 480)
        out.append(_with_entities(m, spec))
    out.append(_real_level())
    for m in out:
        m.setflags(write=False)
    return tuple(out)


def entities(level):
    """[(type, centre x, centre y, orientation)] of a synthetic level in map order, base records included; a door (5, 6, 8) stands at
    the position the ninja has to touch: its switch (6, 8) or itself (5)"""
    m = level_maps()[level]
    out = [(3, 6.0 * m[1236], 6.0 * m[1237], 0), (4, 6.0 * m[1241], 6.0 * m[1242], 0)]
    for e in level_specs()[level]:
        x, y = (e[5], e[6]) if len(e) > 5 else (e[1], e[2])
        out.append((e[0], 6.0 * x, 6.0 * y, e[3]))
    return out


def mover_slot(level, index):
    """slot (entity_dic order: type ascending, map order inside a type) of the index-th record of level_specs()[level]"""
    spec = level_specs()[level]
    order = sorted((k for k, e in enumerate(spec) if e[0] in MOVER_TYPES), key=lambda k: (spec[k][0], k))
    return order.index(index)


def movers(level):
    """[(slot, type, x, y, orientation)] in slot order"""
    spec = level_specs()[level]
    out = [(mover_slot(level, k), e[0], 6.0 * e[1], 6.0 * e[2], e[3]) for k, e in enumerate(spec) if e[0] in MOVER_TYPES]
    return sorted(out)


def orientation_vec(o):
    """physics.py:317-332"""
    sx = 1 if o in (0, 1, 7) else (-1 if 3 <= o <= 5 else 0)
    sy = 1 if 1 <= o <= 3 else (-1 if o >= 5 else 0)
    return (sx * DIAG, sy * DIAG) if o & 1 else (float(sx), float(sy))


def integrated(vx, vy):
    """the speed Ninja.integrate adds to the position at the first tick after a reset"""
    return vx * DRAG, vy * DRAG + GRAVITY


def speed_for(ix, iy):
    """an injected speed whose integrated() is (ix, iy) up to rounding"""
    return ix / DRAG, (iy - GRAVITY) / DRAG


def before(px, py, vx, vy):
    """the injected position from which the first integration with injected speed (vx, vy) lands on (px, py): exactly, where a
    double does (searched over the neighbouring doubles), else the nearest"""
    out = []
    for p, s in zip((px, py), integrated(vx, vy)):
        q = p - s
        best = q
        for k in range(-3, 4):
            c = float(base.ulp_shift(q, k))
            if c + s == p:
                best = c
                break
        out.append(best)
    return out


class _Table:
    def __init__(self):
        self.cols = {k: [] for k in ("level", "xyv", "family", "group", "thr", "mslot", "mxyab", "mfield", "fresh")}
        self.n_groups = 0

    def add(self, level, family, xyv, thr=-1, group=False, axis=0, m0=None, m1=None, fresh=False, maxis=None):
        """one row, or with group=True the 5 ulp-neighbours of the row on ninja coordinate `axis` (or on x of mover 1 when
        maxis is set).  m0, m1: (slot, x, y, a, b, field) or None."""
        ks = range(-2, 3) if group else (0,)
        for k in ks:
            r = [float(v) for v in xyv]
            ms = [list(m) if m is not None else [-1, 0.0, 0.0, 0.0, 0.0, KEEP] for m in (m0, m1)]
            if maxis is not None:
                ms[1][1 + maxis] = float(base.ulp_shift(ms[1][1 + maxis], k))
            else:
                r[axis] = float(base.ulp_shift(r[axis], k))
            c = self.cols
            c["level"].append(level)
            c["xyv"].append(r)
            c["family"].append(family)
            c["group"].append(self.n_groups if group else -1)
            c["thr"].append(thr)
            c["mslot"].append([ms[0][0], ms[1][0]])
            c["mxyab"].append([ms[0][1:5], ms[1][1:5]])
            c["mfield"].append([ms[0][5], ms[1][5]])
            c["fresh"].append(fresh)
        self.n_groups += 1 if group else 0


def _clip(v, vmax):
    n = np.sqrt((v * v).sum(axis=1))
    return v * np.minimum(1.0, vmax / np.maximum(n, 1e-300))[:, None]


def _half_speed(rng, g):
    """v = 0 for every second group, N(0, 0.5) for the rest"""
    return rng.normal(0.0, 0.5, 2) * (g % 2)


def _ball_after_chase(bx, by, nx, ny):
    """where a resting death ball in open space stands after its think() with the ninja at (nx, ny): entity_death_ball.py:80-107"""
    dx, dy = nx - bx, ny - by
    dist = math.sqrt(dx * dx + dy * dy)
    return bx + dx / dist * 0.04, by + dy / dist * 0.04


def _ring_family(T, rng, level):
    ang = 2.0 * np.pi * np.arange(16) / 16.0
    centres = []
    for t, x, y, _ in entities(level):
        if t in (3, 4) and level != PLAIN:   # the exit pair is the same on every level; only PLAIN's stands within one reach
            continue
        centres.append((t, x, y))
    g = 0
    for t, cx, cy in centres:
        for name, R, phase in RING_RADII.get(t, ()):
            if t == 14:
                cx1, cy1 = cx + 8.0 / 7, cy          # the drone's first move: mode 2 keeps dir 0 (entity_drone_base.py:104-124)
            elif t == 26:
                cx1, cy1 = cx, cy + 1.3              # orientation 2: dir 1
            else:
                cx1, cy1 = cx, cy
            # the exit door's ring is reached through its switch 24 px to the left: only the arc within 16 px of that counts
            for a in (math.pi + np.linspace(-0.6, 0.6, 16) if phase == "rest2" else ang):
                for d in RING_D:
                    v = _half_speed(rng, g)
                    g += 1
                    ux, uy = math.cos(a), math.sin(a)
                    px, py = cx1 + (R + d) * ux, cy1 + (R + d) * uy
                    if phase == "pre":
                        T.add(level, RING, [px, py, v[0], v[1]], THR[name], group=True)
                    elif phase == "post":
                        T.add(level, RING, before(px, py, *v) + list(v), THR[name], group=True)
                    elif phase == "leave":
                        # inside 13.5 at the injected position (the mine starts toggling), at 14.5 + d after the first tick
                        ix, iy = (R + d - 13.4) * ux, (R + d - 13.4) * uy
                        T.add(level, RING, [px - ix, py - iy, *speed_for(ix, iy)], THR[name], group=True)
                    elif phase == "rest2":
                        # at rest through the first tick (on the switch), one step of gravity further at the second
                        T.add(level, RING, [px, py - GRAVITY, *speed_for(0.0, 0.0)], THR[name], group=True)
                    elif phase == "ball":
                        # the ball chases the injected position before the ninja integrates: two rounds of the fixed point
                        bx, by = cx, cy
                        for _ in range(3):
                            qx, qy = bx + (R + d) * ux, by + (R + d) * uy
                            inj = before(qx, qy, *v)
                            bx, by = _ball_after_chase(cx, cy, inj[0], inj[1])
                        T.add(level, RING, inj + list(v), THR[name], group=True)


def _square_positions(semi):
    """(dx, dy, axis of the ulp walk) on the four sides at distance `semi`, five places along each, and the four diagonals"""
    out = []
    for side in (-1.0, 1.0):
        for t in (0.0, -7.0, 7.0, -(semi - 0.5), semi - 0.5):
            out.append((side * semi, t, 0))
            out.append((t, side * semi, 1))
    return out


def _square_rows(T, rng, level, family, t, cx, cy, orient, m0=None):
    lo, semi, hi = SQUARE_SEMI[t]
    g = 0
    for name, s in ((lo, semi), (hi, semi + 0.1)):
        for d in RING_D:
            for dx, dy, axis in _square_positions(s + d):
                v = _half_speed(rng, g)
                g += 1
                T.add(level, family, before(cx + dx, cy + dy, *v) + list(v), THR[name], group=True, axis=axis, m0=m0)
    for s in (semi - 1.0, semi - 4.0, semi - 0.05):
        for sx in (-1.0, 1.0):
            for sy in (-1.0, 1.0):
                v = _half_speed(rng, g)
                g += 1
                T.add(level, family, before(cx + sx * s, cy + sy * s, *v) + list(v), THR["square_diagonal"], group=True, m0=m0)
    if t == 20:
        # the kill strip: a segment 11 px ahead of the centre, 7 px each way, radius 12 (entity_thwump.py:221-236); the ninja 19 + e
        # ahead of the centre is (8 + e) from the strip's line, so the strip's ends reach sqrt(144 - (8 + e)^2) further
        horizontal = orient in (0, 4)
        direction = 1.0 if orient in (0, 2) else -1.0
        for e in (0.0, 0.05):
            reach = 7.0 + math.sqrt(144.0 - (8.0 + e) ** 2)
            for end in (-1.0, 1.0):
                for d in RING_D:
                    v = _half_speed(rng, g)
                    g += 1
                    al, ac = direction * (19.0 + e), end * (reach + d)
                    px, py = (cx + al, cy + ac) if horizontal else (cx + ac, cy + al)
                    T.add(level, family, before(px, py, *v) + list(v), THR["thwump_strip_12"], group=True, axis=1 if horizontal else 0, m0=m0)


def _shove_launch_rows(T, level, cx, cy):
    """a resting shove thwump is launched when the logical square (semi-side 22.1) is penetrated and the OTHER axis' penetration
    len2 exceeds 0.2 (entity_shove_thwump.py:185-192).  The ninja stands 22.05 out on one axis -- outside the physical square, 0.05
    inside the logical one: that axis is the shallow one and gives the direction -- and 22.1 - (0.2 + d) out on the other, so len2
    = 0.2 + d; the ulp walk is on that other coordinate.  No random draw: the rows were added after the rest of the table."""
    semi = 12 + 10.0 + 0.1   # as the reference and the kernel compute it
    g = 0
    for d in RING_D:
        for sa in (-1.0, 1.0):
            for sb in (-1.0, 1.0):
                for axis in (0, 1):   # the coordinate that carries len2
                    v = (0.0, 0.0) if g % 2 == 0 else (0.3, -0.2)
                    g += 1
                    shallow, deep = sa * 22.05, sb * (semi - (0.2 + d))
                    dx, dy = (deep, shallow) if axis == 0 else (shallow, deep)
                    T.add(level, SQUARE, before(cx + dx, cy + dy, *v) + list(v), THR["shove_launch_0.2"], group=True, axis=axis)


def _square_family(T, rng, level):
    for t, x, y, o in entities(level):
        if t in SQUARE_SEMI:
            _square_rows(T, rng, level, SQUARE, t, x, y, o)
    for t, x, y, o in entities(level):
        if t == 28:
            _shove_launch_rows(T, level, x, y)


def _oneway_family(T, rng, level):
    for t, cx, cy, o in entities(level):
        if t != 11:
            continue
        nx, ny = orientation_vec(o)
        tx, ty = -ny, nx   # lateral_dist = (dx, dy) . (tx, ty)

        def row(name, lat, nd, nd_old, vt, axis=0):
            # collision position: centre + nd * n + lat * t; integrated speed (nd - nd_old) * n + vt * t
            ix, iy = (nd - nd_old) * nx + vt * tx, (nd - nd_old) * ny + vt * ty
            px, py = cx + nd * nx + lat * tx, cy + nd * ny + lat * ty
            T.add(level, ONEWAY, [px - ix, py - iy, *speed_for(ix, iy)], THR[name], group=True, axis=axis)

        for d in RING_D:
            for sgn in (-1.0, 1.0):
                for vt in (-0.5, 0.5):
                    for axis in (0, 1):
                        row("oneway_lateral_17.1", sgn * (17.1 + d), 9.5, 9.8, vt, axis)
                        row("oneway_lateral_21.1", sgn * (21.1 + d), 9.5, 9.8, vt, axis)
            for lat in (0.0, 8.0, -8.0):
                for axis in (0, 1):
                    row("oneway_normal_0", lat, 0.0 + d, 9.2, 0.3, axis)
                    row("oneway_normal_10", lat, 10.0 + d, 10.3, -0.3, axis)
                    row("oneway_old_8.9", lat, 8.5, 8.9 + d, 0.3, axis)
                    row("oneway_old_8.9", lat, 9.2, 8.9 + d, -0.3, axis)   # normal_proj > 0: never collides


def _pad_family(T, rng, level):
    boosts = []
    for t, cx, cy, o in entities(level):
        if t == 10:
            nx, ny = orientation_vec(o)
            tx, ty = -ny, nx
            g = 0
            for d in RING_D:
                for lat in (0.0, 6.0, -6.0, 11.0, -11.0):
                    for axis in (0, 1):
                        v = _half_speed(rng, g)
                        g += 1
                        px, py = cx + (10.1 + d) * nx + lat * tx, cy + (10.1 + d) * ny + lat * ty
                        T.add(level, PAD, before(px, py, *v) + list(v), THR["launch_plane_10.1"], group=True, axis=axis)
        elif t == 24:
            boosts.append((cx, cy))
    if len(boosts) == 2:
        mx, my = (boosts[0][0] + boosts[1][0]) / 2, (boosts[0][1] + boosts[1][1]) / 2
        for dx, dy in ((0.0, 0.0), (3.0, 4.0), (-5.0, 9.0), (0.0, -14.0), (2.0, 14.8)):   # all inside both 16 px rings (pads 12 apart)
            for v in ((0.0, 0.0), (-0.0, 0.0), (5e-324, 0.0), (0.0, -1e-200), (1e-170, 1e-170), (0.3, -0.2), (-2.0, 0.0)):
                T.add(level, PAD, [mx + dx, my + dy, v[0], v[1]], THR["boost_speed_0"], group=True)


def _lane_family(T, rng, level):
    for t, cx, cy, o in entities(level):
        if t != 20:
            continue
        horizontal = o in (0, 4)
        direction = 1 if o in (0, 2) else -1
        along0 = cx if horizontal else cy
        tc0 = math.floor((along0 - direction * 11) / 12)
        bound = 12.0 * tc0 if direction == 1 else 12.0 * (tc0 + 1)

        def row(name, along, across, axis_along):
            x, y = (along, cy + across) if horizontal else (cx + across, along)
            axis = (0 if horizontal else 1) if axis_along else (1 if horizontal else 0)
            T.add(level, LANE, [x, y, 0.0, 0.0], THR[name], group=True, axis=axis)

        for sgn in (-1.0, 1.0):
            for d in RING_D:
                for ahead in (40.0, 100.0):
                    row("lane_38", along0 + direction * ahead, sgn * (38.0 + d), False)
            for across in (0.0, 30.0, 37.9):
                for k in (0, 1, -1):   # the face cell's bound and the 12 px bounds next to it
                    row("lane_cell", bound + 12.0 * k, sgn * across, True)


def _uniform(T, rng, level, family, n, sigma):
    x = rng.uniform(24.0, 1032.0, n)
    y = rng.uniform(24.0, 576.0, n)
    v = _clip(rng.normal(0.0, sigma, (n, 2)), V_MAX)
    for k in range(n):
        T.add(level, family, [x[k], y[k], v[k, 0], v[k, 1]])


def _ball_slot(level):
    if level == REAL:
        from nclone_amd.engine import compile_level_zoo

        return [k for k, r in enumerate(compile_level_zoo(level_maps()[REAL])[2]) if r[0] == 25]
    return [s for s, t, _, _, _ in movers(level) if t == 25]


def _ball_uniform(T, rng, level, family, n, sigma):
    slot = _ball_slot(level)[0]
    x = rng.uniform(24.0, 1032.0, n)
    y = rng.uniform(24.0, 576.0, n)
    v = _clip(rng.normal(0.0, sigma, (n, 2)), 60.0)
    for k in range(n):
        T.add(level, family, [SPAWN[0], SPAWN[1], 0.0, 0.0], m0=(slot, x[k], y[k], v[k, 0], v[k, 1], KEEP))


def _ball_lattice(T, rng, level, n_groups):
    """inject_states._lattice_family's anchoring (three groups in four at an end point of a segment of the compiled table, -1..1
    lattice steps away) with the ball's own offsets"""
    from nclone_amd.engine import compile_level_segments

    slot = _ball_slot(level)[0]
    seg = compile_level_segments(level_maps()[level])[0].astype(np.int64)
    seg = seg[(seg[:, 2] == 0) & (seg[:, 0] >= 1) & (seg[:, 0] <= 42) & (seg[:, 1] >= 1) & (seg[:, 1] <= 23)]
    pick = seg[rng.integers(0, len(seg), n_groups)]
    end = rng.integers(0, 2, n_groups)
    step = np.array([-1, 0, 0, 1])
    i = np.where(end == 0, pick[:, 3], pick[:, 5]) // 12 + step[rng.integers(0, 4, n_groups)]
    j = np.where(end == 0, pick[:, 4], pick[:, 6]) // 12 + step[rng.integers(0, 4, n_groups)]
    free = np.arange(n_groups) % 4 == 0
    i = np.where(free, rng.integers(2, 87, n_groups), np.clip(i, 2, 86))
    j = np.where(free, rng.integers(2, 49, n_groups), np.clip(j, 2, 48))
    off = np.array(BALL_OFFSETS)
    x = 12.0 * i + off[rng.integers(0, len(off), n_groups)]
    y = 12.0 * j + off[rng.integers(0, len(off), n_groups)]
    x[2::8] = 12.0 * i[2::8]   # every eighth group exactly on the lattice point: on the segment's end
    y[2::8] = 12.0 * j[2::8]
    v = rng.normal(0.0, 0.5, (n_groups, 2)) * (np.arange(n_groups) % 2)[:, None]
    for g in range(n_groups):
        # a resting ball gets the chase term: the speed that cancels it keeps a v = 0 group on its point
        if g % 4 == 2:
            dx, dy = SPAWN[0] - x[g], SPAWN[1] - y[g]
            dist = math.sqrt(dx * dx + dy * dy)
            v[g] = (-(dx / dist * 0.04), -(dy / dist * 0.04))
        T.add(level, BALL_LATTICE, [SPAWN[0], SPAWN[1], 0.0, 0.0], group=True, maxis=(g // 2) % 2,
              m1=(slot, x[g], y[g], v[g, 0], v[g, 1], KEEP))


def _ball_speed(T, rng, level):
    slot = _ball_slot(level)[0]
    pre_135 = (1.35 - 0.85) / 0.9 + 0.85   # the speed the clamp (entity_death_ball.py:95-101) maps to 1.35
    for s in (0.85, 0.85 + 0.01 / 0.9, 1.35, pre_135):
        for d in (0.0, 1e-7, -1e-7, 1e-9, -1e-9, 1e-12, -1e-12, 1e-15, -1e-15):
            for x in (40.0, 55.5, 71.0, 86.5, 102.0):
                for ang in (math.pi / 2, math.pi / 3, 2 * math.pi / 3):   # into the floor, straight and slanted
                    y = base.FLOOR_TOP - 7.5
                    dx, dy = SPAWN[0] - x, SPAWN[1] - y
                    dist = math.sqrt(dx * dx + dy * dy)
                    vx, vy = (s + d) * math.cos(ang) - dx / dist * 0.04, (s + d) * math.sin(ang) - dy / dist * 0.04
                    T.add(level, BALL_SPEED, [SPAWN[0], SPAWN[1], 0.0, 0.0], m0=(slot, x, y, vx, vy, KEEP))


def _ball_pair(T, rng, level):
    s0, s1 = _ball_slot(level)
    ang = 2.0 * np.pi * np.arange(16) / 16.0
    bx, by = 300.0, 450.0   # open space
    ax, ay = _ball_after_chase(bx, by, *SPAWN)
    for a in ang:
        for d in RING_D:
            T.add(level, BALL_PAIR, [SPAWN[0], SPAWN[1], 0.0, 0.0], group=True, maxis=0, fresh=True, m0=(s0, bx, by, 0.0, 0.0, KEEP),
                  m1=(s1, ax + (16.0 + d) * math.cos(a), ay + (16.0 + d) * math.sin(a), 0.0, 0.0, KEEP))


def _thwump_family(T, rng, level):
    for slot, t, x0, y0, o in movers(level):
        if t != 20:
            continue
        horizontal = o in (0, 4)
        direction = 1.0 if o in (0, 2) else -1.0
        origin = x0 if horizontal else y0

        def put(along, state, ninja=(SPAWN[0], SPAWN[1], 0.0, 0.0), other=None):
            other = (y0 if horizontal else x0) if other is None else other
            x, y = (along, other) if horizontal else (other, along)
            T.add(level, THWUMP, list(ninja), m0=(slot, x, y, 0.0, 0.0, state))

        back, fwd = 8.0 / 7, 20.0 / 7
        # (a) retreating within a step of the origin, from both sides, and on it
        for f in (0.0, 1e-9, 0.25, 0.5, 1 - 1e-9, 1.0, 1 + 1e-9, 1.5, 2.0):
            for side in (1.0, -1.0):
                put(origin + side * direction * back * f, -1)
        # (b) the leading edge (11 px ahead) within a step of a 12 px bound: a free one in open space, the map's border (blocked)
        wall = {0: 1032.0, 2: 576.0, 4: 24.0, 6: 24.0}[o]
        free = 12.0 * math.floor(origin / 12.0) + direction * 60.0
        for bound in (free, wall):
            for f in (-1e-9, 0.0, 1e-9, 0.5, 1 - 1e-9, 1.0, 1 + 1e-9, 1.5):
                put(bound - direction * (11.0 + fwd * f), 1)
        # ... and retreating with the trailing edge at a free bound
        for f in (-1e-9, 0.0, 1e-9, 0.5, 1 - 1e-9, 1.0, 1 + 1e-9):
            put(free + direction * (11.0 + back * f), -1)
        # (c) crushing (ninja.py:531-537) needs a face that does not kill, the trailing one: a thwump in state -1 moves against its
        # charging direction until blocked, wherever its origin is.  The ninja stands between that face and the floor (o = 6: charges
        # up, retreats down) or the left wall at floor level (o = 0), the gap around the ninja's 20 px; 8 / 7 px per tick
        if o == 6:
            for gap in np.linspace(-2.0, 8.0, 41):
                for nx in (72.0, 60.5):
                    put(base.FLOOR_TOP - 20.0 - 9.0 - gap, -1, ninja=(nx, base.FLOOR_TOP - 10.0, 0.0, 0.0), other=72.0)
        if o == 0:
            for gap in np.linspace(-2.0, 8.0, 41):
                put(24.0 + 20.0 + 9.0 + gap, -1, ninja=(34.0, base.FLOOR_TOP - 10.0, 0.0, 0.0), other=base.FLOOR_TOP - 10.0)
        # ... and the charging face at the same places: it kills on touch (entity_thwump.py:221-240)
        if o == 2:
            for gap in np.linspace(-2.0, 14.0, 9):
                put(base.FLOOR_TOP - 20.0 - 9.0 - gap, 1, ninja=(72.0, base.FLOOR_TOP - 10.0, 0.0, 0.0), other=72.0)


def _drone_family(T, rng, level):
    for slot, t, x0, y0, o in movers(level):
        if t not in (14, 26):
            continue
        speed = 8.0 / 7 if t == 14 else 1.3
        for d in range(4):
            vx, vy = (1, 0, -1, 0)[d], (0, 1, 0, -1)[d]
            for delta in (0.0, 5e-7, 1e-6 - 1e-12, 1e-6, 1e-6 + 1e-12, 2e-6, 0.5 * speed, speed * (1 - 1e-9), speed, speed * (1 + 1e-9),
                          2.5 * speed, -1e-6, -0.5 * speed):
                T.add(level, DRONE, [SPAWN[0], SPAWN[1], 0.0, 0.0], m0=(slot, x0 - vx * delta, y0 - vy * delta, x0, y0, d))


def _bounce_family(T, rng, level, n):
    for slot, t, x0, y0, o in movers(level):
        if t != 17:
            continue
        for _ in range(n):
            r, a = rng.uniform(0.0, 40.0), rng.uniform(0.0, 2 * math.pi)
            x, y = x0 + r * math.cos(a), y0 + r * math.sin(a)
            vx, vy = rng.normal(0.0, 3.0, 2)
            # entity_bounce_block.py:107-122: where the block stands when the ninja collides
            wx, wy = vx * 0.98, vy * 0.98
            cx, cy = x + wx, y + wy
            cx, cy = cx + 0.02222222222222222 * (x0 - cx), cy + 0.02222222222222222 * (y0 - cy)
            m0 = (slot, x, y, vx, vy, KEEP)
            for name, s in (("bounce_19", 19.0), ("bounce_19.1", 19.1)):
                side = rng.integers(0, 4)
                tpos = rng.uniform(-s + 1, s - 1)
                dx, dy, axis = ((-s, tpos, 0), (s, tpos, 0), (tpos, -s, 1), (tpos, s, 1))[side]
                v = _half_speed(rng, _)
                T.add(level, BOUNCE, before(cx + dx, cy + dy, *v) + list(v), THR[name], group=True, axis=axis, m0=m0)


@functools.lru_cache(maxsize=None)
def states():
    """dict of read-only arrays, rows ordered by level, inside a level by family:
    level i32 [n], xyv f64 [n, 4], family i32 [n], group i32 [n] (-1: none), thr i32 [n] (index into THRESHOLDS, -1: none),
    mslot i32 [n, 2] (-1: no mover written), mxyab f64 [n, 2, 4], mfield i32 [n, 2] (KEEP: state / dir left alone), fresh bool [n]"""
    rng = np.random.default_rng(SEED)
    T = _Table()
    for level in (PLAIN, STATIC, MOVERS, BALLS):
        _ring_family(T, rng, level)
        _square_family(T, rng, level)
        _oneway_family(T, rng, level)
        _pad_family(T, rng, level)
        _lane_family(T, rng, level)
        _uniform(T, rng, level, FREE, N_FREE, 3.0)
        _uniform(T, rng, level, FAST, N_FAST, 45.0)
        if level in (MOVERS, BALLS):
            _ball_uniform(T, rng, level, BALL_FREE, N_BALL_FREE, 1.0)
            _ball_uniform(T, rng, level, BALL_FAST, N_BALL_FAST, 20.0)
        if level == MOVERS:
            _ball_lattice(T, rng, level, N_BALL_LATTICE_GROUPS)
            _ball_speed(T, rng, level)
            _thwump_family(T, rng, level)
            _drone_family(T, rng, level)
            _bounce_family(T, rng, level, N_BOUNCE)
        if level == BALLS:
            _ball_pair(T, rng, level)
    _uniform(T, rng, REAL, FREE, N_FREE, 3.0)
    _uniform(T, rng, REAL, FAST, N_FAST, 45.0)
    _ball_uniform(T, rng, REAL, BALL_FREE, N_BALL_FREE, 1.0)   # most of this level is solid: the 16-iteration cap
    _ball_uniform(T, rng, REAL, BALL_FAST, N_BALL_FAST, 20.0)
    dt = {"level": np.int32, "xyv": np.float64, "family": np.int32, "group": np.int32, "thr": np.int32, "mslot": np.int32,
          "mxyab": np.float64, "mfield": np.int32, "fresh": bool}
    out = {k: np.array(v, dtype=dt[k]) for k, v in T.cols.items()}
    order = np.lexsort((np.arange(len(out["level"])), out["family"], out["level"]))
    out = {k: v[order] for k, v in out.items()}
    assert np.isfinite(out["xyv"]).all() and np.isfinite(out["mxyab"]).all()
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def inputs():
    """uint8 [TICKS, n] replay input bytes (bit 0 jump, bit 1 right, bit 2 left), one seeded random byte per state and tick; the rows
    of an ulp-neighbour group share their first row's bytes, so that nothing but the walked coordinate differs inside a group."""
    group = states()["group"]
    n = len(group)
    a = np.random.default_rng(SEED + 1).integers(0, 8, size=(TICKS, n)).astype(np.uint8)
    first = np.arange(n)
    g = group >= 0
    _, start, inverse = np.unique(group[g], return_index=True, return_inverse=True)
    first[g] = np.nonzero(g)[0][start][inverse]
    a = np.ascontiguousarray(a[:, first])
    a.setflags(write=False)
    return a


N_MOVERS_MAX = 12   # mover rows recorded per state (the REAL level is chosen to fit)
_ORACLE = {}


def oracle_run(om, variant):
    """The oracle's run of every row: dict of read-only arrays F f64 [n, TICKS, 12], D i32 [n, TICKS, 22], C f64 [n, TICKS, 6] (entity
    checksum), E i32 [n, TICKS, 64] (entity_words: the packing of NppBatch.dump_entities, -1 past the level's count), M f64 [n, TICKS, N_MOVERS_MAX, 5]
    (dump_movers, NaN past the level's count), B i32 [n, TICKS, 4] (Oracle.ball_debug of that tick), valid bool [n, TICKS]: no
    earlier tick left the row terminal.  Computed once per variant and shared."""
    if variant not in _ORACLE:
        s = states()
        inp = inputs()
        n = len(s["level"])
        F = np.zeros((n, TICKS, 12), dtype=np.float64)
        D = np.zeros((n, TICKS, 22), dtype=np.int32)
        Cs = np.zeros((n, TICKS, 6), dtype=np.float64)
        E = np.full((n, TICKS, 64), -1, dtype=np.int32)
        M = np.full((n, TICKS, N_MOVERS_MAX, 5), np.nan, dtype=np.float64)
        B = np.zeros((n, TICKS, 4), dtype=np.int32)
        hor_jump = [om.controls(b) for b in range(8)]
        for lv, m in enumerate(level_maps()):
            o = om.Oracle(variant)
            o.load(m)
            assert o.unsupported == 0 and len(o.dump_movers()) <= N_MOVERS_MAX and len(o.entity_words()) <= 64
            dirty = False   # the simulator has been reset since its load
            for k in np.nonzero(s["level"] == lv)[0]:
                if s["fresh"][k]:
                    if dirty:
                        o.load(m)
                        dirty = False
                else:
                    o.reset()
                dirty = True
                o.set_ninja(*s["xyv"][k])
                for j in range(2):
                    if s["mslot"][k, j] >= 0:
                        f = int(s["mfield"][k, j])
                        o.set_mover(int(s["mslot"][k, j]), *s["mxyab"][k, j], None if f == KEEP else f)
                o.ball_debug()
                for t in range(TICKS):
                    o.tick(*hor_jump[inp[t, k]])
                    f, d = o.core()
                    F[k, t], D[k, t] = f, d[:22]
                    Cs[k, t] = o.entity_checksum()
                    e = o.entity_words()
                    E[k, t, :len(e)] = e
                    mv = o.dump_movers()
                    M[k, t, :len(mv)] = mv
                    B[k, t] = o.ball_debug()
        terminal = np.isin(D[:, :, 0], (6, 7, 8))
        valid = np.ones((n, TICKS), dtype=bool)
        valid[:, 1:] = ~(np.cumsum(terminal, axis=1)[:, :-1] > 0)
        out = {"F": F, "D": D, "C": Cs, "E": E, "M": M, "B": B, "valid": valid}
        for a in out.values():
            a.setflags(write=False)
        _ORACLE[variant] = out
    return _ORACLE[variant]


# strides without a common factor with the 5 values of RING_D, so that the picked groups keep every d
GOLDEN_STRIDE = {RING: 9, SQUARE: 9, ONEWAY: 19, PAD: 9, LANE: 7, FREE: 10, FAST: 10, BALL_FREE: 10, BALL_FAST: 10, BALL_LATTICE: 7,
                 BALL_SPEED: 7, BALL_PAIR: 9, THWUMP: 3, DRONE: 2, BOUNCE: 4}


def golden_subset():
    """Indices into states() of the rows the reference fixture tests/golden/inject_zoo.npz holds: every GOLDEN_STRIDE-th row of each
    (level, family), or every GOLDEN_STRIDE-th ulp-neighbour group, whole, where the family has groups -- by position in the table
    alone."""
    s = states()
    pick = []
    for lv in range(len(LEVEL_NAMES)):
        for f, stride in GOLDEN_STRIDE.items():
            idx = np.nonzero((s["level"] == lv) & (s["family"] == f))[0]
            if not len(idx):
                continue
            g = s["group"][idx]
            if (g >= 0).all():
                idx = idx[(g - g.min()) % stride == 0]
            else:
                assert (g < 0).all()
                idx = idx[::stride]
            pick.append(idx)
    return np.concatenate(pick)
