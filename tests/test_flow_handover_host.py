"""The task table of the data-flow reduced solve against the waits of the hand-over THROUGH COLUMN i-2 (csrc/sfm_ba_flow.h), host
side, no GPU.  The closer of row i forms L[i][i-3] as before, then waits for W_i-2 and finishes the row: L[i][i-2] and the blocks
(i, i-1) and (i, i) through column i-2.  It reads the hand-over task's block of its own row, L[i-1][i-3] and the finished block
(i-1, i-2) of the closer above (row 3: the chain's L[2][0] and L[2][1]).  The chain's preparation waves only copy rows r >= 3."""
import pytest

T1, CLOSER, H1, RHS, IDENT, CAMSUM, SRED, COST = range(8)
NB = 32
NBKS = [2, 3, 4, 5, 6, 11, 44, 52]
CAMS = {2: 9, 3: 10, 4: 14, 5: 19, 6: 23, 11: 50, 44: 200, 52: 237}      # a camera count with that many block columns


# A flag is named by what it announces: ("W", k), ("X", e, m), ("L", i, k), ("y", k), ("cam", c, part), ("S", i, k, q), ("cost",),
# ("h", i, 1) block (i, i-1) through column i-4, ("h", i, 0) the same block through column i-2, ("h", i, 2) block (i, i) through i-2.
def chain_publishes(nbk, j):
    out = [("W", j), ("X", j, j)]
    if j + 1 < nbk:
        out.append(("L", j + 1, j))
        if j == 1:
            out.append(("L", 2, 0))          # row 2 has no closer
    return out


def chain_waits(nbk, j, n_cams):
    r, out = j + 1, []
    if j == 0 and n_cams:
        out += [("cam", c, part) for c in range(min(n_cams - 1, (NB - 1) // 7) + 1) for part in range(4)]
    if r < nbk:
        if r >= 3:
            out += [("h", r, 0), ("h", r, 2)]
        elif n_cams:
            out += [("S", r, k, q) for k in range(r + 1) for q in range(4)]
    return out


def closer_reads(i):
    """(waits before L[i][i-3] is announced, waits behind it) of the closer of row i, S apart."""
    c = i - 3
    first = [f for m in range(c - 1) for f in (("L", c, m), ("L", i - 2, m), ("L", i, m))]
    if c >= 1:
        first += [("L", c, c - 1), ("L", i, c - 1), ("L", i - 2, c - 1)]
    first += [("W", c), ("L", i - 2, c)]
    second = [("L", i - 1, c), ("h", i, 1)] + ([("h", i - 1, 0)] if i >= 4 else []) + [("W", i - 2)] + ([("L", 2, 1)] if i == 3 else [])
    return first, second


def task_steps(nbk, n_cams, ty, i, k, key):
    """A task as a list of (waits, publishes) steps in the order the kernel takes them."""
    sred = n_cams > 0
    last = nbk - 1

    def cams_of_rows(row0, row1):
        return range(row0 // 7, min(n_cams - 1, row1 // 7) + 1)

    def dp(e):
        return [("X", e, m) for m in range(e, nbk)] + [("y", m) for m in range(e, nbk)] + ([("cost",)] if sred else [])

    def s_blocks(row, k0, k1):
        return [("S", row, b, q) for b in range(k0, k1 + 1) for q in range(4)] if sred else []

    if ty == T1:
        return [(s_blocks(i, k, k) + [f for m in range(k) for f in (("L", k, m), ("L", i, m))] + [("W", k)], [("L", i, k)])]
    if ty == H1:
        return [(s_blocks(i, i - 1, i - 1) + [f for m in range(i - 3) for f in (("L", i - 1, m), ("L", i, m))], [("h", i, 1)])]
    if ty == CLOSER:
        first, second = closer_reads(i)
        return [(s_blocks(i, i - 3, i) + first, [("L", i, i - 3)]), (second, [("L", i, i - 2), ("h", i, 0), ("h", i, 2)])]
    if ty == RHS:
        w = [("cam", c, part) for c in cams_of_rows(NB * k, min(7 * n_cams - 1, NB * k + NB - 1)) for part in range(4)] if sred else []
        w += [f for m in range(k) for f in (("L", k, m), ("y", m))] + [("W", k)]
        steps = [(w, [("y", k)])]
        if k == last:
            steps.append((dp(last), []))
        return steps
    if ty == IDENT:
        steps = [([f for m in range(i, k) for f in (("L", k, m), ("X", i, m))] + [("W", k)], [("X", i, k)])]
        if k == last:
            steps.append((dp(i), []))
        return steps
    if ty == CAMSUM:
        return [([], [("cam", i, k)])]
    if ty == SRED:
        q = key & 3
        return [([("cam", c, part) for c in cams_of_rows(NB * i + 8 * q, NB * i + 8 * q + 7) for part in range(4)] if k >= i - 1 else [], [("S", i, k, q)])]
    assert ty == COST
    return [([], [("cost",)])]


def tables(sfm, nbk):
    yield 0, sfm.native.flow_tasks(nbk).tolist()
    n_cams = CAMS[nbk]
    assert (7 * n_cams + NB - 1) // NB == nbk
    yield n_cams, sfm.native.flow_tasks_deferred(n_cams).tolist()


@pytest.mark.parametrize("nbk", NBKS)
def test_closer_comes_after_everything_it_reads(sfm, nbk):
    for n_cams, table in tables(sfm, nbk):
        assert len(table) > 0
        keys = [r[3] >> 2 for r in table]      # (the two low bits of a task that sums S name its quarter of the block)
        assert keys == sorted(keys)
        pos = {}
        for n, (ty, i, k, key) in enumerate(table):
            for _, pubs in task_steps(nbk, n_cams, ty, i, k, key):
                for f in pubs:
                    assert f not in pos, ("two producers", f)
                    pos[f] = n
        chain = {f for j in range(nbk) for f in chain_publishes(nbk, j)}
        assert not (chain & set(pos))
        closers = [(n, r[1]) for n, r in enumerate(table) if r[0] == CLOSER]
        assert [i for _, i in closers] == list(range(3, nbk))
        for n, i in closers:
            assert pos[("h", i, 1)] < n                                  # the hand-over task of its own row
            if i >= 4:
                assert pos[("h", i - 1, 0)] < n and pos[("L", i - 1, i - 3)] == pos[("h", i - 1, 0)]      # the closer of row i-1
            first, second = closer_reads(i)
            blocks = [f for f in first + second if f[0] == "L"]
            for row in (i, i - 1, i - 2):                                # every block of L of these rows that it reads
                for f in blocks:
                    if f[1] == row:
                        assert f in chain or pos[f] < n, (f, n)
            for f in first + second:
                assert f in chain or pos[f] < n, (f, n)


@pytest.mark.parametrize("nbk", NBKS)
def test_one_task_workgroup_and_a_chain_fed_by_hand_overs_terminate(sfm, nbk):
    """The chain and ONE task workgroup that takes the table strictly in order, each blocked by its waits; the chain advances a
    step only when the hand-over of the row it prepares has been delivered."""
    for n_cams, table in tables(sfm, nbk):
        steps = [st for (ty, i, k, key) in table for st in task_steps(nbk, n_cams, ty, i, k, key)]
        published = {f for _, pubs in steps for f in pubs} | {f for j in range(nbk) for f in chain_publishes(nbk, j)}
        for waits, _ in steps:
            assert set(waits) <= published
        for j in range(nbk):
            assert set(chain_waits(nbk, j, n_cams)) <= published
        up, t, j = set(), 0, 0
        while t < len(steps) or j < nbk:
            moved = False
            while t < len(steps) and all(f in up for f in steps[t][0]):
                up.update(steps[t][1]); t += 1; moved = True
            while j < nbk and all(f in up for f in chain_waits(nbk, j, n_cams)):
                up.update(chain_publishes(nbk, j)); j += 1; moved = True
            assert moved, ("deadlock", nbk, n_cams, steps[t][0] if t < len(steps) else None, j)


def test_the_walk_finds_a_closer_ahead_of_its_hand_over_task(sfm):
    """Not vacuous: with the closer of row 3 ahead of the hand-over task of row 3 the single task workgroup stalls."""
    nbk = 5
    table = sfm.native.flow_tasks(nbk).tolist()
    c3 = next(n for n, r in enumerate(table) if r[0] == CLOSER and r[1] == 3)
    h3 = next(n for n, r in enumerate(table) if r[0] == H1 and r[1] == 3)
    assert h3 < c3
    table.insert(h3, table.pop(c3))
    steps = [st for (ty, i, k, key) in table for st in task_steps(nbk, 0, ty, i, k, key)]
    up, t, j = set(), 0, 0
    while True:
        moved = False
        while t < len(steps) and all(f in up for f in steps[t][0]):
            up.update(steps[t][1]); t += 1; moved = True
        while j < nbk and all(f in up for f in chain_waits(nbk, j, 0)):
            up.update(chain_publishes(nbk, j)); j += 1; moved = True
        if not moved:
            break
    assert t < len(steps) and j < nbk
