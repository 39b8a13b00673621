"""The control of the list merges' chunked walk (k_merge_spec, lasp_amd/csrc/
laspj_lists.hip), restated in plain Python over two lists of key ranks: the launch shape
merge_enqueue gives it, each chunk's walk from its entry column per round, the round's
decision (settled / another round / fall back to the one-wave walk), and the features of
the final round's walk that decide which branches of the plan writer run.  Nothing else of
the kernel is restated — windows, streams and the plan's layout are the device's business;
tests/test_gpu_spec_walk.py compares what it writes with the oracle.

A walk of rows [i0, i1) of A from column j of B is the clauses' own two-finger walk
(oracle/otp.py orddict_merge / ordsets_union) cut at row i1: skip B[j] < A[i] (the B item
goes first, alone), pair on equality, else the row goes alone; it stops once row i1 - 1 is
placed.  Rounds are counted as the kernel's `round` after its increment: a walk that
settles at round index k took k + 1 rounds (never fewer than 2, never more than 15); a
fall at `rounds` == 16 is the cap, an earlier one the majority rule."""

from dataclasses import dataclass, field

WAVES = 4            # kSpW: chunks (waves) per workgroup
ROUNDS = 16          # kSpRounds
DEFAULT_CHUNK = 1024

NOT_LAUNCHED, SETTLED, FELL = 0, 1, 2      # laspj_ctx_last_list_walk's values


def launch(known_e, knob=0, R=1, walk=3):
    """(L, C, grid) of the launch, or None when merge_enqueue launches no chunked walk
    (walk: LASPJ_TUNE_LIST_WALK — 3 forces it for R <= 4, 1 forbids it; the hint-driven
    default is the caller's to decide)."""
    if known_e == 0 or R > 4 or walk == 1:
        return None
    L = max(knob or DEFAULT_CHUNK, -(-known_e // 1024))
    if L >= 1 << 20:
        return None
    C = -(-(-(-known_e // L)) // WAVES) * WAVES
    return L, C, C // WAVES


def descends(xs):
    return any(x > y for x, y in zip(xs, xs[1:]))


def chunk_walk(A, B, i0, i1, entry, steps=None):
    """Rows [i0, i1) of A from column `entry` of B: (exit column, pairs, last single side
    — 0 none, 1 A, 2 B).  steps (a list): every step appended as ("A", i, j), ("B", i, j)
    or ("P", i, j) with the state (i, j) it was taken from."""
    nb = len(B)
    i, j, pairs, side = i0, entry, 0, 0
    while i < i1:
        if j >= nb:                                   # B is done: rows alone
            if steps is not None:
                steps.extend(("A", k, j) for k in range(i, i1))
            i, side = i1, 1
            break
        x, y = A[i], B[j]
        if x == y:
            if steps is not None:
                steps.append(("P", i, j))
            pairs, i, j = pairs + 1, i + 1, j + 1
        elif x < y:
            if steps is not None:
                steps.append(("A", i, j))
            i, side = i + 1, 1
        else:
            if steps is not None:
                steps.append(("B", i, j))
            j, side = j + 1, 2
    return j, pairs, side


@dataclass
class Walk:
    outcome: int                    # NOT_LAUNCHED / SETTLED / FELL (this replica's)
    walked: bool = False            # the replica's keys descend: the kernel walks it
    rounds: int = 0
    fell_by: str = ""               # "majority" / "cap"
    L: int = 0
    C: int = 0
    grid: int = 0
    nc: int = 0                     # chunks with rows
    words: list = field(default_factory=list)     # final round: (entry, exit, pairs, side)
    steps: list = field(default_factory=list)     # final round's chunk walks, concatenated
    chunk_steps: list = field(default_factory=list)
    history: list = field(default_factory=list)   # per round: blocks changed


def run(A, B, knob=0, known_e=None, R=1, walk=3):
    """One replica's (A, B) under the launch known_e / knob / R give (known_e: the longest
    A of the batch; default len(A))."""
    na, nb = len(A), len(B)
    shape = launch(na if known_e is None else known_e, knob, R, walk)
    if shape is None:
        return Walk(NOT_LAUNCHED)
    L, C, grid = shape
    nc = -(-na // L)
    w = Walk(SETTLED, L=L, C=C, grid=grid, nc=nc)
    if not (descends(A) or descends(B)):
        return w                                     # launched; this replica skips it
    w.walked = True
    memo = {}

    def one(c, entry):
        if (c, entry) not in memo:
            memo[c, entry] = chunk_walk(A, B, c * L, min(na, c * L + L), entry)
        return memo[c, entry]

    prev, rnd = None, 0
    while True:
        cur = []
        for c in range(nc):
            entry = 0 if c == 0 else (c * L * nb // na if rnd == 0 else prev[c - 1][1])
            cur.append((entry,) + one(c, entry))
        changed = 0
        if rnd > 0:
            for blk in range(grid):
                cs = range(blk * WAVES, min(nc, blk * WAVES + WAVES))
                changed += any(cur[c][1] != prev[c][1] for c in cs)
        w.history.append(changed)
        prev = cur
        if rnd > 0 and changed == 0:
            break
        rnd += 1
        if rnd == ROUNDS or (rnd > 1 and 2 * changed > grid):
            w.outcome, w.rounds = FELL, rnd
            w.fell_by = "cap" if rnd == ROUNDS else "majority"
            return w
    w.rounds = rnd + 1
    w.words = prev
    for c in range(nc):
        st = []
        chunk_walk(A, B, c * L, min(na, c * L + L), prev[c][0], st)
        w.chunk_steps.append(st)
        w.steps += st
    return w


def batch_outcome(walks):
    """laspj_ctx_last_list_walk after a call whose replicas' walks are `walks`."""
    if any(w.outcome == NOT_LAUNCHED for w in walks):
        return NOT_LAUNCHED
    return FELL if any(w.outcome == FELL for w in walks) else SETTLED


def merged(w, na, nb, gset=False):
    """The merge the settled walk's plan describes, as the clauses emit it: a list of
    ("A", i), ("B", j) and ("P", i, j, side) — side (G-Set lists, ordsets:union's argument
    switch): 1 the pair's item is A's, 2 B's: the side of the last single step before it,
    A at the start.  After the last row, B's tail."""
    out, side = [], 1
    for k, i, j in w.steps:
        if k == "P":
            out.append(("P", i, j, side if gset else 1))
        else:
            out.append((k, i) if k == "A" else (k, j))
            side = 1 if k == "A" else 2
    j = w.words[-1][1] if w.words else 0
    out.extend(("B", k) for k in range(j, nb))
    return out


def features(w, na, nb):
    """What the final round's walk of a settled replica exercises (a dict of counts and
    flags; see tests/test_spec_walk_model.py test_table_reaches_every_branch)."""
    f = dict(chunks=w.nc, blocks=w.grid, rounds=w.rounds, full_last=na % w.L == 0,
             idle_waves=w.nc % WAVES != 0, tie_cross=False, a_cross=False, b_at_boundary=False,
             b_at_group=False, longest_b=0, b_runs=set(), allpair_then_pair=0, entered_b_done=False)
    run_b = 0
    for k, _i, _j in w.steps:                         # (a B run ends at the row it precedes)
        if k == "B":
            run_b += 1
        elif run_b:
            f["b_runs"].add(run_b)
            run_b = 0
    f["longest_b"] = max(f["b_runs"], default=0)
    last_side = 0                                     # of the last chunk with one, before c
    for c, st in enumerate(w.chunk_steps):
        entry = w.words[c][0]
        if entry >= nb:
            f["entered_b_done"] = True
        if c > 0 and st and w.chunk_steps[c - 1]:
            a, b = w.chunk_steps[c - 1][-1][0], st[0][0]
            f["tie_cross"] |= a == "P" and b == "P"
            f["a_cross"] |= a == "A" and b == "A" and entry < nb
            f["b_at_boundary"] |= b == "B"
            # the carried side must come from the last chunk that has one, not from the
            # chunk before: that one only paired, an earlier one ended on a B step, and
            # this chunk opens with pairs (their item is B's in a G-Set merge)
            if b == "P" and w.words[c - 1][3] == 0 and last_side == 2:
                lead = 0
                while lead < len(st) and st[lead][0] == "P":
                    lead += 1
                f["allpair_then_pair"] = max(f["allpair_then_pair"], lead)
        # a B run before the first row of a later 64-row group of the chunk
        for s, (k, i, _j) in enumerate(st):
            if k == "B" and i > c * w.L and (i - c * w.L) % 64 == 0 and st[s - 1][0] != "B":
                f["b_at_group"] = True
        if w.words[c][3]:
            last_side = w.words[c][3]
    return f
