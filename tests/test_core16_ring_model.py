"""Host model of the fp32 core's weight ring (csrc/mlp_core16.h, WeightPipe16T) with the sub-stage stagger of the SIMD partners (LAG).

Eight waves walk the same fragment stream.  Each wave's program is written down event by event from the kernel's source -- piece issue,
LDS read (V16_AHEAD fragments ahead), use (the MFMAs), s_waitcnt vmcnt + s_barrier -- and a scheduler interleaves the waves in adversarial
orders: one wave runs until the barrier stops it, then the next; the early half (waves 0..3) as far ahead as the barrier allows, the late half
(waves 4..7) as far behind, each late wave behind the other late waves, and seeded random interleavings.  Two properties are asserted at every
event, with the LDS-DMA taken at both of its extremes:

  refill         a piece is issued only when every wave has consumed the fragment it overwrites (the DMA may land at once);
  certification  a fragment is read only when its owner has waited for the piece (vmcnt) in front of a barrier the reader has passed
                 (the DMA may land as late as the owner's wait allows).

The model must pass for LAG 0, 2, 4, 6 and must see the hazard at LAG 8 (the static_assert in the header refuses that build)."""
import random

import pytest

# mirrored constants -- csrc/mlp_core.h:18 (RING_SLOTS), csrc/layout.h (STAGE_FRAGS = 16 fragments of 1 KiB), csrc/mlp_core16.h:24-26
# (V16_WAVES, V16_PIECES, V16_AHEAD) and the members of WeightPipe16T: SYNC_S, LATE_S, EARLY_P0/P1, LATE_P0/P1, SYNC_VMCNT, LATE_VMCNT
RING_SLOTS = 6
STAGE_FRAGS = 16
V16_WAVES = 8
V16_PIECES = STAGE_FRAGS // V16_WAVES
V16_AHEAD = 4
SYNC_S = STAGE_FRAGS - 2
SYNC_VMCNT = V16_PIECES * (RING_SLOTS - 4)
LATE_VMCNT = V16_PIECES * (RING_SLOTS - 5)
START_VMCNT = V16_PIECES * (RING_SLOTS - 3)      # WeightPipe16T::start
EARLY_P = (4, 10)


class RingHazard(AssertionError):
    pass


def program(wave, lag, stages, late_pieces=None):
    """The events of one wave, in program order: ("issue", stage, frag) | ("wait", n) | ("barrier",) | ("read", stage, frag) | ("use", stage, frag)."""
    late = wave >= 4                                  # WeightPipe16T::start: stagger = (wave >> 2) & 1
    late_s = SYNC_S - lag
    if late_pieces is None:
        late_pieces = (late_s, late_s + 2)
    ev = []
    for c in range(RING_SLOTS - 1):                   # start(): RING_SLOTS - 1 stages of pieces, then the first certification
        for i in range(V16_PIECES):
            ev.append(("issue", c, 2 * wave + i))
    ev += [("wait", START_VMCNT), ("barrier",)]
    for f in range(V16_AHEAD):                        # prime()
        ev.append(("read", 0, f))
    for c in range(stages):
        for s in range(0, STAGE_FRAGS, 2):
            # before_step(s)
            if lag == 0:
                if s % 4 == 0 and ((s >> 2) & 1) == int(late):
                    ev.append(("issue", c + RING_SLOTS - 1, 2 * wave + (s >> 3)))
            else:
                if late and s == late_s:
                    ev += [("wait", LATE_VMCNT), ("barrier",)]
                pos = late_pieces if late else EARLY_P
                if s in pos:
                    ev.append(("issue", c + RING_SLOTS - 1, 2 * wave + pos.index(s)))
            # mma_layer16: the look-ahead reads, then the MFMAs
            for f in (s + V16_AHEAD, s + 1 + V16_AHEAD):
                ev.append(("read", c + f // STAGE_FRAGS, f % STAGE_FRAGS))
            ev += [("use", c, s), ("use", c, s + 1)]
            # after_step(s)
            if s == SYNC_S and (lag == 0 or not late):
                ev += [("wait", SYNC_VMCNT), ("barrier",)]
    return ev


def run(lag, order, stages=3 * RING_SLOTS + 2, late_pieces=None):
    """Steps the eight programs under `order` (a function: runnable waves, program counters -> the wave that executes its next event)."""
    progs = [program(w, lag, stages, late_pieces) for w in range(V16_WAVES)]
    assert len({sum(e[0] == "barrier" for e in p) for p in progs}) == 1, "every wave passes the same number of barriers"
    pc = [0] * V16_WAVES
    arrived = [None] * V16_WAVES                       # index of the barrier the wave waits at
    passed = [0] * V16_WAVES                           # barriers completed
    used = [set() for _ in range(V16_WAVES)]           # (stage, frag) consumed
    flight = [[] for _ in range(V16_WAVES)]            # pieces in flight, issue order
    landed = [[] for _ in range(V16_WAVES)]            # waited for, not yet behind a barrier of the owner
    certified = {}                                     # (stage, frag) -> index of the barrier that certifies it
    while True:
        runnable = [w for w in range(V16_WAVES) if arrived[w] is None and pc[w] < len(progs[w])]
        if not runnable:
            if all(a is None for a in arrived):
                return
            raise RingHazard("deadlock: %r" % (arrived,))
        w = order(runnable, pc)
        e = progs[w][pc[w]]
        pc[w] += 1
        if e[0] == "issue":
            _, st, f = e
            old = st - RING_SLOTS
            if old >= 0:
                for r in range(V16_WAVES):
                    if (old, f) not in used[r]:
                        raise RingHazard("refill: wave %d overwrites fragment %d of stage %d (with stage %d) before wave %d has consumed it" % (w, f, old, st, r))
            flight[w].append((st, f))
        elif e[0] == "wait":
            while len(flight[w]) > e[1]:
                landed[w].append(flight[w].pop(0))
        elif e[0] == "barrier":
            for piece in landed[w]:
                certified[piece] = passed[w]           # the barrier this wave is about to arrive at
            landed[w] = []
            arrived[w] = passed[w]
            if all(a is not None for a in arrived):
                assert len(set(arrived)) == 1
                for r in range(V16_WAVES):
                    arrived[r] = None
                    passed[r] += 1
        elif e[0] == "read":
            _, st, f = e
            if certified.get((st, f), 1 << 30) >= passed[w]:
                raise RingHazard("certification: wave %d reads fragment %d of stage %d, which no barrier it has passed certifies" % (w, f, st))
        else:
            used[w].add((e[1], e[2]))


def by_priority(prio):
    return lambda runnable, pc: min(runnable, key=prio.index)


ORDERS = {
    "early_half_ahead": by_priority([0, 1, 2, 3, 4, 5, 6, 7]),        # each wave runs to its barrier; wave 7 is always the last to arrive
    "late_half_ahead": by_priority([4, 5, 6, 7, 0, 1, 2, 3]),
    "reversed": by_priority([7, 6, 5, 4, 3, 2, 1, 0]),
    "partners_apart": by_priority([3, 7, 2, 6, 1, 5, 0, 4]),
    "lockstep": lambda runnable, pc: min(runnable, key=lambda w: pc[w]),      # the wave that is furthest behind goes next
}


def _random_order(seed):
    rng = random.Random(seed)
    return lambda runnable, pc: rng.choice(runnable)


def _all_orders():
    for name, o in ORDERS.items():
        yield name, o
    for seed in range(6):
        yield "random%d" % seed, _random_order(seed)


@pytest.mark.parametrize("lag", [0, 2, 4, 6])
def test_ring_is_safe(lag):
    for name, order in _all_orders():
        run(lag, order)


def test_the_model_sees_the_refill_hazard_at_lag_8():
    """LATE_S = 6: behind b_(c-1) an early wave rewrites fragments 0..7 while a late wave has consumed 0..5 only."""
    with pytest.raises(RingHazard, match="refill"):
        run(8, ORDERS["early_half_ahead"])
    failing = 0
    for name, order in _all_orders():
        try:
            run(8, order)
        except RingHazard:
            failing += 1
    assert failing >= 1


@pytest.mark.parametrize("lag", [2, 4, 6])
def test_late_pieces_at_the_unstaggered_positions_are_a_hazard(lag):
    """Why the late half issues its pieces behind its own rendezvous: at the LAG = 0 positions (steps 4 and 12) a late wave rewrites fragments
    8..15 of slot(c-1) when b_(c-1) has only told it that the other late waves consumed stage c - 1 below LATE_S."""
    with pytest.raises(RingHazard, match="refill"):
        run(lag, ORDERS["early_half_ahead"], late_pieces=(4, 12))


def test_the_model_sees_a_short_vmcnt_wait():
    """Certification.  A stage is certified two barriers before it is first read, so the late rendezvous has two whole stages of slack:
    with up to 2 * V16_PIECES more pieces in flight than LATE_VMCNT allows the model still passes, in every order; with one piece more than
    that (five more than LATE_VMCNT) a fragment is read that no passed barrier certifies -- in every order, asserted order by order."""
    global LATE_VMCNT
    keep = LATE_VMCNT
    try:
        LATE_VMCNT = keep + 2 * V16_PIECES
        for name, order in _all_orders():
            run(6, order)
        LATE_VMCNT = keep + 2 * V16_PIECES + 1
        for name, order in _all_orders():
            with pytest.raises(RingHazard, match="certification"):
                run(6, order)
    finally:
        LATE_VMCNT = keep


def test_header_constants_match_the_model():
    """The mirrored constants are the ones the header states."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cr-nerf-pytorch_amd", "csrc")
    core, core16 = open(os.path.join(csrc, "mlp_core.h")).read(), open(os.path.join(csrc, "mlp_core16.h")).read()
    assert re.search(r"constexpr int RING_SLOTS = %d;" % RING_SLOTS, core)
    assert re.search(r"constexpr int V16_WAVES = %d;" % V16_WAVES, core16)
    assert re.search(r"constexpr int V16_AHEAD = %d;" % V16_AHEAD, core16)
    assert "EARLY_P0 = %d, EARLY_P1 = %d;" % EARLY_P in core16
    assert "LATE_P0 = LATE_S, LATE_P1 = LATE_S + 2;" in core16
    assert "SYNC_VMCNT = V16_PIECES * (RING_SLOTS - 4);" in core16 and "LATE_VMCNT = V16_PIECES * (RING_SLOTS - 5);" in core16
    assert "static_assert(LATE_S >= STAGE_FRAGS / 2" in core16
