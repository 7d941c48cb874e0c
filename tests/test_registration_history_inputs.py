"""What tests/test_gpu_registration_history.py rests on, asserted on the CPU (tests/registration_history.py): the size list really
crosses the capacities it is meant to cross, on every path that re-allocates, and the launch plans along the sequence really
reuse a captured graph across sizes, really turn real partial rows into padding, really grow the partial block late."""
import collections
import os
import re
import subprocess

import pytest

import registration_history as RH

ROOT = RH.ROOT
REALLOC = ("past", "jump")


def test_capacity_rule_is_read_from_the_source_and_the_list_follows_it():
    assert set(RH.capacity_rule()) <= set("L0123456789 +*/()")       # an integer expression in L, evaluated as C evaluates it
    if RH.capacity_rule() == "(L + L / 8 + 255) / 256 * 256":         # (today's rule: a scan more than one eighth larger re-allocates)
        assert [RH.c(L) for L in (1, 256, 257, 512, 513, 3400)] == [256, 512, 512, 768, 768, 3840]
    assert all(RH.c(L) >= L and RH.c(L + 1) >= RH.c(L) for L in range(1, 5000))
    a, b = RH.c(1), RH.c(RH.c(1) + 1)
    assert 1 < a and a + 1 < b                                         # the list's small entries are five different sizes
    assert RH.sizes() == (1, a, a + 1, b, b + 1, 65, RH.FULL, 64, 1, a + 1, RH.FULL_LESS_ONE) and len(RH.sizes()) == RH.N_SIZES
    # the other constants the simulation restates
    src = open(RH.CAPI_HIP).read()
    assert re.search(r"static constexpr int kStreamSlots = %d;" % RH.N_STREAM_SLOTS, src)
    assert "if (&other != &sl && !other.pending) RC_TRY(prepare_slot(" in src      # a submission sizes every idle slot
    assert "doubles = std::max(doubles, (size_t)2 * 288 * kAcc * 8);" in src       # the floor of ensure_partials
    assert ("return align_up(((size_t)2 * n_scans * prows * kAcc + (size_t)2 * n_scans * grid + kAcc) * sizeof(double)) / sizeof(double);"
            in src)                                                                # partial_doubles_of, restated in tests/cpp
    assert "key = key * 1000003ll + shapes[h].grid * 64ll + shapes[h].batch;" in src  # the geometry key: (grid, batch)


def test_scene_is_the_small_one():
    pb = RH.problem()
    assert len(pb.kf_trees) == 9 and len(pb.leaves) == 3
    for q in range(RH.N_QUERIES):
        assert 4000 <= pb.q_scans[q].shape[0] <= 4800 and 2500 <= RH.l_full(q) <= 4000, (pb.q_scans[q].shape, RH.l_full(q))
        assert RH.l_full(q) - 1 > RH.c(RH.c(1) + 1) + 1           # the whole scan is a jump up from every small entry
    assert len({RH.l_full(q) for q in range(RH.N_QUERIES)}) == RH.N_QUERIES


def test_the_sequence_meets_every_kind_with_every_entry_of_the_list():
    assert len(RH.STEPS) == 66 and [k for _, k, _ in RH.STEPS[:6]] == list(RH.KINDS)
    import math
    assert math.gcd(RH.N_SIZES, len(RH.K_CYCLE)) == 1 and math.gcd(RH.N_SIZES, len(RH.B_CYCLE)) == 1
    assert math.gcd(len(RH.K_CYCLE), len(RH.B_CYCLE)) == 1
    first = collections.defaultdict(set)
    for _, kind, n in RH.STEPS:
        sp = RH.spec_of(kind, n)
        for batch in sp.batches:
            q, L = batch[0]
            first[kind] |= {e for e in RH.sizes() if RH.size_of(e, q) == L}
        # a batch's scans differ in size (the list holds two sizes twice: eight entries in a row may hold both of them twice)
        assert all(len({L for _, L in batch}) >= min(len(batch), max(2, len(batch) - 2)) for batch in sp.batches)
        if len(sp.batches) == 2:
            assert [L for _, L in sp.batches[0]] != [L for _, L in sp.batches[1]]             # ... and so do batches in flight
        if kind == "stream":
            assert sp.Ks[0] != sp.Ks[1]
        if kind == "stream_tree":
            assert len({RH.moving_tree(q, s).num_leaves for q, s in sp.strides}) == 2
    for kind in RH.KINDS:
        assert first[kind] == set(RH.sizes()), (kind, first[kind])
    assert {sp.Ks[0] for sp in RH.specs()} == set(RH.K_CYCLE)
    for kind in ("batch", "pipelined"):
        assert {len(RH.spec_of(kind, n).batches[0]) for n in range(RH.N_SIZES)} == set(RH.B_CYCLE)
    assert sum(sp.mid is not None for sp in RH.specs()) == 1


def test_the_size_list_crosses_the_capacities_on_every_path():
    events, _ = RH.census()
    count = collections.Counter((path, w) for _, _, path, w in events)
    realloc = {p: sum(count[p, w] for w in REALLOC) for p in ("update", "update_async", "slot", "slot_idle")}
    print("re-allocations per path:", realloc, "exact fits:", {p: count[p, "exact"] for p in ("update", "update_async", "slot")})
    assert realloc["update"] >= 3 and realloc["update_async"] >= 2 and realloc["slot"] >= 2 and realloc["slot_idle"] >= 1
    per_kind = collections.defaultdict(collections.Counter)
    for _, kind, _, w in events:
        per_kind[kind][w] += 1
    for kind in RH.KINDS:
        assert per_kind[kind]["exact"] >= 1 and per_kind[kind]["past"] >= 1 and per_kind[kind]["fits"] >= 1, (kind, per_kind[kind])
    # "a large buffer used small": every path ends on buffers that hold a whole scan and are given a single leaf
    assert count["update", "jump"] >= 3 and count["update_async", "jump"] >= 1 and count["slot", "jump"] + count["slot_idle", "jump"] >= 1


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "registration_history_plan")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "mad_icp_amd", "csrc", "common"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "registration_history_plan.cpp"),
                           "-o", exe])
    _, launches = RH.census()
    floor, rows = RH.plans(launches, exe)
    return launches, floor, rows


def test_launch_plans_along_the_sequence(planned):
    launches, floor, rows = planned
    assert floor == 2 * 288 * 30 * 8 == 138240
    # the issue's three probes of make_plan
    by_shape = {(l.batch, l.K, l.max_L): r for l, r in zip(launches, rows)}
    assert by_shape[1, 1, 1][0] == 8
    assert any(g == 256 for (B, K, L), (g, _, _) in by_shape.items() if B == 1 and K == 9 and L >= 2500)
    assert all(d >= 138400 for (B, _, _), (_, d, _) in by_shape.items() if B == 8)
    # graph reuse across L: two launches in a row under one graph key — the plan and the Job array (the batch's, or a stream
    # slot's) — with different L.  (A linearisation is never captured: allow_graph = false.)
    last, reuse = {}, []
    for l, (_, _, tie) in zip(launches, rows):
        if l.kind == "linearize":
            continue
        key = (tie, l.slot)
        if key in last and last[key].max_L != l.max_L:
            reuse.append((last[key].step, l.step, last[key].max_L, l.max_L))
        last[key] = l
    # consecutive steps of the sequence with equal plans and different L (whatever the Job array)
    adjacent = [(a.step, b.step) for (a, ra), (b, rb) in zip(zip(launches, rows), list(zip(launches, rows))[1:])
                if ra[2] == rb[2] and a.max_L != b.max_L]
    # stale rows that become padding: grid 256 directly followed by grid 8 at the same batch size
    shrink = [(a.step, b.step) for (a, ra), (b, rb) in zip(zip(launches, rows), list(zip(launches, rows))[1:])
              if ra[0] == 256 and rb[0] == 8 and a.batch == b.batch]
    # the partial block grows after graphs exist, with a ticket pending: the batch in the middle of the stream step is the FIRST
    # launch that needs more than the floor
    over = [i for i, (_, d, _) in enumerate(rows) if d > floor]
    print("plan-equal pairs under one graph key:", len(reuse), "adjacent launches with equal plans:", len(adjacent),
          "grid 256 -> 8 at equal batch:", len(shrink), "launches above the floor:", len(over), "first at step", launches[over[0]].step)
    assert len(reuse) >= 1 and len(adjacent) >= 1 and len(shrink) >= 1
    assert over and over[0] > 0 and launches[over[0]].kind == "batch(mid)"
    assert any(l.kind in ("register", "batch", "pipelined") for l in launches[:over[0]])      # (graphs exist by then)
    assert max(d for _, d, _ in rows[:over[0]]) <= floor < rows[over[0]][1]
    # the geometry key changes often: most launches zero the block anew
    keys = [(g, l.batch) for l, (g, _, _) in zip(launches, rows)]
    assert sum(a != b for a, b in zip(keys, keys[1:])) >= 20
