"""The ring's hop schedule as a pure function: no process group, no tensors.

For every world size 1..9, both modes and every rank: each other rank's chunk
arrives exactly once, in the expected number of hops, and what a rank sends in
a direction at a hop is what the neighbour on that side expects to receive."""

import pytest

from distributed_sigmoid_loss_amd.parallel.ring import ring_schedule

CASES = [(w, bidir) for w in range(1, 10) for bidir in (False, True)]


@pytest.mark.parametrize("world,bidir", CASES)
def test_schedule_visits_every_other_rank_once(world, bidir):
    for rank in range(world):
        seen = [src for hop in ring_schedule(world, rank, bidir)
                for src in (hop.from_right, hop.from_left) if src is not None]
        assert sorted(seen) == [r for r in range(world) if r != rank]


@pytest.mark.parametrize("world,bidir", CASES)
def test_schedule_hop_count(world, bidir):
    want = -(-(world - 1) // 2) if bidir else world - 1
    for rank in range(world):
        assert len(ring_schedule(world, rank, bidir)) == want


@pytest.mark.parametrize("world,bidir", CASES)
def test_schedule_send_matches_neighbour_receive(world, bidir):
    sched = [ring_schedule(world, r, bidir) for r in range(world)]
    for rank in range(world):
        right, left = (rank + 1) % world, (rank - 1) % world
        for k, hop in enumerate(sched[rank]):
            # None on both sides when the hop does not use the direction
            assert hop.send_right == sched[right][k].from_left
            assert hop.send_left == sched[left][k].from_right
            # a rank can only forward a chunk it already holds
            held = {rank} | {s for h in sched[rank][:k]
                             for s in (h.from_right, h.from_left)}
            assert {hop.send_right, hop.send_left} - {None} <= held


def test_schedule_arrival_order_and_labels():
    """Own block first is the caller's; then per bidirectional round right
    before left, then the remainder — with the span labels HopStats keys on."""
    hops = ring_schedule(4, 1, bidir=True)
    assert [(h.from_right, h.from_left) for h in hops] == [(2, 0), (None, 3)]
    assert [(h.wait_label, h.loss_label) for h in hops] == [
        ("ring_bhop1_wait", "ring_bchunk1_loss"), ("ring_rem_wait", None)]
    # the remainder hop forwards the rightward-travelling stream
    assert (hops[1].send_right, hops[1].send_left) == (0, None)
    hops = ring_schedule(3, 1, bidir=False)
    assert [h.from_left for h in hops] == [0, 2]
    assert [(h.wait_label, h.loss_label) for h in hops] == [
        ("ring_hop1_wait", "ring_chunk1_loss"),
        ("ring_hop2_wait", "ring_chunk2_loss")]
