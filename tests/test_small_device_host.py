"""Launch plans at small compute-unit counts, host side (no GPU): the compute-unit limit hook (sfm_set_cu_limit), the grid of
the data-flow reduced solve, a simulation of its task table with ONE task workgroup next to the chain -- what a 32-CU partition
of an MI355X launches at the largest sizes -- and the group width `group` = 0 stands for under a limit."""
import pytest

T1, CLOSER, H1, RHS, IDENT, CAMSUM, SRED, COST = range(8)
NB = 32                                  # rows of a block column of the reduced system (kNB)


@pytest.fixture(autouse=True)
def _no_limit_left_behind(sfm):
    yield
    sfm.native.set_cu_limit(0)
    dev, eff = sfm.native.cu_count()
    assert eff == dev


def flow_grid_before(n_cus, n_tasks):
    """The launch size before the clamp: 1 + min(ntasks, num_cus - 32)."""
    return 1 + min(n_tasks, n_cus - 32)


@pytest.mark.parametrize("n_tasks", [1, 5, 3000])
@pytest.mark.parametrize("n_cus", [1, 2, 16, 32, 33, 40, 41, 64, 128, 256, 304])
def test_flow_grid_has_a_task_workgroup_and_fits_the_device(sfm, n_cus, n_tasks):
    grid = sfm.native.flow_grid(n_cus, n_tasks)
    if n_cus >= 2:
        assert 2 <= grid <= max(2, n_cus)        # the chain and at least one task workgroup, one CU each (121 KB of LDS)
    else:
        assert grid == 0                         # no such launch: the column steps (ba_flow_setup)
    assert grid - 1 <= n_tasks
    if n_cus > 40:
        assert grid == flow_grid_before(n_cus, n_tasks)


def test_flow_grid_of_empty_or_negative_arguments(sfm):
    assert sfm.native.flow_grid(0, 5) == 0 and sfm.native.flow_grid(-3, 5) == 0 and sfm.native.flow_grid(64, 0) == 0


# ---- the task table, run by one task workgroup -------------------------------------------------------------------------
# Restated from the waits of csrc/sfm_ba_flow.h.  A flag is named by what it announces:
#   ("W", k)  W_k = L_kk^-1          ("X", e, m)  block m of identity row e     ("L", i, k)  block (i, k) of L
#   ("y", k)  block k of the rhs row ("h", i, t)  hand-over block (i, i-2+t)    ("cam", c, part), ("S", i, k, q), ("cost",)
def chain_publishes(nbk, j):
    """What step j of the chain announces, all of it behind the step's workgroup barrier: W_j and X_j, the block (r, r-2) of the
    row r = j+1 it prepared, and L[j+1][j]."""
    out = [("W", j), ("X", j, j)]
    if j + 1 < nbk:
        out.append(("L", j + 1, j))
        if j >= 1:
            out.append(("L", j + 1, j - 1))
    return out


def chain_waits(nbk, j, n_cams):
    """What step j of the chain waits for: its preparation waves take over row r = j+1 -- the three hand-over blocks from r = 3
    on -- before the barrier that W_j is announced behind.  With the reduce deferred (n_cams > 0) the chain sums D_0 itself once
    the camera sums of block row 0 are there, and reads rows 1 and 2 of S as the SRED tasks publish them."""
    r, out = j + 1, []
    if j == 0 and n_cams:
        out += [("cam", c, part) for c in range(min(n_cams - 1, (NB - 1) // 7) + 1) for part in range(4)]
    if r < nbk:
        if r >= 3:
            out += [("h", r, 0), ("h", r, 1), ("h", r, 2)]
        elif n_cams:
            out += [("S", r, k, q) for k in range(r + 1) for q in range(4)]
    return out


def cams_of_rows(row0, row1, n_cams):
    return range(row0 // 7, min(n_cams - 1, row1 // 7) + 1)


def task_waits(nbk, n_cams, ty, i, k, key):
    """Every flag the task waits for, and what it publishes."""
    sred = n_cams > 0
    last = nbk - 1

    def dp(e):      # the workgroup that finishes identity row e (or y) forms dp_e; the last to arrive waits for the cost
        return [("X", e, m) for m in range(e, nbk)] + [("y", m) for m in range(e, nbk)] + ([("cost",)] if sred else [])

    def s_blocks(row, k0, k1):
        return [("S", row, b, q) for b in range(k0, k1 + 1) for q in range(4)] if sred else []

    if ty == T1:
        return (s_blocks(i, k, k) + [f for m in range(k) for f in (("L", k, m), ("L", i, m))] + [("W", k)], [("L", i, k)])
    if ty == H1:
        return (s_blocks(i, i - 1, i - 1) + [f for m in range(i - 3) for f in (("L", i - 1, m), ("L", i, m))], [("h", i, 1)])
    if ty == CLOSER:
        c = i - 3
        w = s_blocks(i, c, i)
        w += [f for m in range(c - 1) for f in (("L", c, m), ("L", i - 2, m), ("L", i, m))]
        if c >= 1:
            w += [("L", c, c - 1), ("L", i, c - 1), ("L", i - 2, c - 1)]
        w += [("W", c), ("L", i - 2, c)]
        return (w, [("L", i, c), ("h", i, 0), ("h", i, 2)])
    if ty == RHS:
        w = [("cam", c, part) for c in cams_of_rows(NB * k, min(7 * n_cams - 1, NB * k + NB - 1), n_cams) for part in range(4)] if sred else []
        w += [f for m in range(k) for f in (("L", k, m), ("y", m))] + [("W", k)]
        if k == last:
            w += [f for f in dp(last) if f != ("y", last)]
        return (w, [("y", k)])
    if ty == IDENT:
        w = [f for m in range(i, k) for f in (("L", k, m), ("X", i, m))] + [("W", k)]
        if k == last:
            w += [f for f in dp(i) if f != ("X", i, last)]
        return (w, [("X", i, k)])
    if ty == CAMSUM:
        return ([], [("cam", i, k)])
    if ty == SRED:
        q = key & 3
        w = [("cam", c, part) for c in cams_of_rows(NB * i + 8 * q, NB * i + 8 * q + 7, n_cams) for part in range(4)] if k >= i - 1 else []
        return (w, [("S", i, k, q)])
    assert ty == COST
    return ([], [("cost",)])


def simulate_one_worker(nbk, table, n_cams=0):
    """The chain and ONE task workgroup that takes the table strictly in order: a task begun is finished before the next is
    taken, and a wait blocks the workgroup.  Returns the last chain step every solve task waited for directly.  Progress is
    monotone (a flag once up stays up), so the order in which the two are advanced does not matter."""
    producers = {}
    for j in range(nbk):
        for f in chain_publishes(nbk, j):
            assert f not in producers, f
            producers[f] = ("chain", j)
    parsed = []
    for n, (ty, i, k, key) in enumerate(table):
        waits, pubs = task_waits(nbk, n_cams, ty, i, k, key)
        for f in pubs:
            assert f not in producers, ("two producers", f)
            producers[f] = ("task", n)
        parsed.append((waits, pubs))
    for n, (waits, _) in enumerate(parsed):       # nothing waits for a flag nobody raises
        for f in waits:
            assert f in producers, ("task %d %r waits for %r, which nobody publishes" % (n, table[n], f))
    for j in range(nbk):
        for f in chain_waits(nbk, j, n_cams):
            assert f in producers, ("chain step %d waits for %r, which nobody publishes" % (j, f))

    up, t, j = set(), 0, 0
    while t < len(parsed) or j < nbk:
        moved = False
        while t < len(parsed) and all(f in up for f in parsed[t][0]):
            up.update(parsed[t][1]); t += 1; moved = True
        while j < nbk and all(f in up for f in chain_waits(nbk, j, n_cams)):
            up.update(chain_publishes(nbk, j)); j += 1; moved = True
        if not moved:
            missing_t = [f for f in parsed[t][0] if f not in up] if t < len(parsed) else []
            missing_c = [f for f in chain_waits(nbk, j, n_cams) if f not in up] if j < nbk else []
            pytest.fail("deadlock with one task workgroup at nbk=%d: task %d %r waits for %r, chain step %d for %r"
                        % (nbk, t, table[t] if t < len(parsed) else None, missing_t[:4], j, missing_c[:4]))
    last_chain = []
    for (waits, _) in parsed:
        steps = [producers[f][1] for f in waits if producers[f][0] == "chain"]
        last_chain.append(max(steps) if steps else -1)
    return last_chain


@pytest.mark.parametrize("nbk", list(range(2, 53)))
def test_task_table_can_be_run_by_one_task_workgroup(sfm, nbk):
    """On 2 .. 40 compute units the launch may have a single task workgroup (at 32 CUs with 52 block columns: 1 + 31 at most, but
    any number down to one must do: the table is taken by tickets).  The table must then be runnable strictly in order beside the
    chain.  Also pinned: the sort key names the chain column a task waits for last (64 x column + place)."""
    table = sfm.native.flow_tasks(nbk).tolist()
    assert len(table) > 0
    last_chain = simulate_one_worker(nbk, table)
    for (ty, i, k, key), col in zip(table, last_chain):
        if ty == H1:
            assert col == -1 and key // 64 == max(0, i - 4)      # waits for tasks only: the closer of row i-1, column i-4
        elif ty == RHS and k == nbk - 1:
            assert col == nbk - 1 and key // 64 == nbk - 1
        else:
            assert col == key // 64 == (i - 3 if ty == CLOSER else k), (ty, i, k, key, col)


@pytest.mark.parametrize("n_cams", [9, 19, 37, 74, 237])
def test_task_table_with_the_reduce_deferred_can_be_run_by_one_task_workgroup(sfm, n_cams):
    nbk = (7 * n_cams + NB - 1) // NB
    table = sfm.native.flow_tasks_deferred(n_cams).tolist()
    assert len(table) > 0
    simulate_one_worker(nbk, table, n_cams)


def test_the_simulation_finds_a_table_in_the_wrong_order(sfm):
    """The check above is not vacuous: the same table with the closer of row 3 moved behind the task that needs its block stalls."""
    nbk = 6
    table = sfm.native.flow_tasks(nbk).tolist()
    n = next(q for q, r in enumerate(table) if r[0] == CLOSER and r[1] == 3)
    table.append(table.pop(n))
    with pytest.raises(pytest.fail.Exception, match="deadlock"):
        simulate_one_worker(nbk, table)


# ---- the hook --------------------------------------------------------------------------------------------------------
def test_cu_limit_argument_rules(sfm):
    native = sfm.native
    lib = native.load()
    dev, eff = native.cu_count()
    assert dev >= 1 and eff == dev
    assert lib.sfm_set_cu_limit(-1) == native.E_SHAPE and "negative" in native.last_error()
    assert native.cu_count() == (dev, dev)
    with pytest.raises(ValueError):
        native.set_cu_limit(-7)
    for n in (1, 2, 32, 33, dev):
        native.set_cu_limit(n)
        assert native.cu_count() == (dev, min(n, dev))
    native.set_cu_limit(dev + 1000)                  # never above the device's own count
    assert native.cu_count() == (dev, dev)
    native.set_cu_limit(0)
    assert native.cu_count() == (dev, dev)
    assert lib.sfm_cu_count(None, None) == native.OK
    assert lib.sfm_version() >= 109


# ---- group = 0 under a limit -------------------------------------------------------------------------------------------
WIDTHS = (1, 4, 8, 16, 32, 64)


def auto_group_rule(n_pts, max_track, n_cus):
    """the narrowest width whose lanes keep the longest track in registers (6 observations each), widened
    while the call gives the device fewer than two waves per SIMD (8 per CU) and the next width is no wider than that track."""
    i = 0
    while i < 5 and not 6 * WIDTHS[i] >= max_track:
        i += 1
    while i < 5 and n_pts * WIDTHS[i] // 64 < 8 * n_cus and WIDTHS[i + 1] <= max_track:
        i += 1
    return WIDTHS[i]


@pytest.mark.parametrize("limit", [1, 32, 256])
def test_auto_group_width_follows_the_effective_cu_count(sfm, limit):
    native = sfm.native
    native.set_cu_limit(limit)
    _, eff = native.cu_count()
    assert eff == min(limit, native.cu_count()[0])
    picked = {}
    for (n_pts, n_obs, max_track) in ((1, 2, 2), (100, 300, 3), (40, 2000, 64), (600, 9000, 40), (3000, 30000, 40), (5000, 20000, 12),
                                      (20000, 160000, 64), (200000, 800000, 7)):
        got = native.tracks_auto_group(n_pts, n_obs, max_track)
        assert got == auto_group_rule(n_pts, max_track, eff), (n_pts, n_obs, max_track, eff)
        picked[(n_pts, max_track)] = got
    # the cases are chosen so that the limit matters: a scene that fills one CU's SIMDs, not 32 or 256 CUs'
    if eff == 1:
        assert picked[(600, 40)] == 8 and picked[(3000, 40)] == 8
    elif eff == 32:
        assert picked[(600, 40)] == 32 and picked[(3000, 40)] == 8
    elif eff == 256:
        assert picked[(600, 40)] == 32 and picked[(3000, 40)] == 32
