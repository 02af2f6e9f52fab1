"""The attention launch plan (csrc/attn_plan.h) on the CPU, through the host-emulation library's ace_mi_attn_plan /
ace_mi_attn_plan_block / ace_mi_attn_plan_tiles (pure functions, no device).

tests/golden/attn_plans.json was written by launch_attention's policy block as it stood before the plan existed (the
split / tail / kernel rules, the two grid expressions and the merge selection, copied into a stand-alone program with
the statics and the device query as parameters), over head shapes x tile counts x block counts x CU counts on both
sides of every threshold in the rules and over every policy setting.  The literal cases below are written by hand from
the rules' comments and the GPU tests, so that a rule change has to be made twice, on purpose.  The property checks
hold whatever the rules say: every grid covers every (block, part) once, and a block's parts tile its key range."""
import ctypes
import json
import os

import pytest

from hostlib import CLANG, build_host_lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_plans.json")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(CLANG):
        pytest.skip("host clang++ not available")
    return ctypes.CDLL(build_host_lib())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def capi():
    from acestep_mi355x import capi
    return capi


def test_plans_match_golden(lib, golden):
    c = capi()
    assert tuple(golden["shape_columns"]) == c.ATTN_SHAPE_FIELDS
    assert tuple(golden["policy_columns"]) == c.ATTN_POLICY_FIELDS
    assert tuple(golden["row_columns"]) == ("shape", "policy") + c.ATTN_PLAN_FIELDS
    assert len(golden["rows"]) >= 2000
    bad = []
    for si, pi, *want in golden["rows"]:
        shape, policy = golden["shapes"][si], dict(zip(c.ATTN_POLICY_FIELDS, golden["policies"][pi]))
        p = c.attn_plan(shape, lib=lib, **policy)
        got = [p[n] for n in c.ATTN_PLAN_FIELDS[:5]] + [c.ATTN_KERNELS.index(p["kernel"]), c.ATTN_MERGES.index(p["merge"]),
                                                        p["merge_grid"]]
        if got != want:
            bad.append((shape, policy, want, got))
    assert not bad, bad[:10]


def test_golden_lies_on_both_sides_of_the_rules(golden):
    """The grid the golden was written over: every CU count, GQA ratio, policy setting and plan kind occurs."""
    pol = golden["policies"]
    assert {p[5] for p in pol} == {8, 20, 256, 304}
    assert {p[0] for p in pol} == {0, 1, 2, 3, 4} and {p[1] for p in pol} == {0, 1} and {p[2] for p in pol} == {16, 8, 2}
    assert {p[3] for p in pol} == {0, 1} and {p[4] for p in pol} == {-1, 0, 1}
    sh = golden["shapes"]
    assert {s[1] // s[2] for s in sh} == {1, 2, 4} and {s[5] for s in sh} == {0, 128} and {s[7] for s in sh} == {0, 1}
    assert {-(-s[4] // 64) for s in sh if s[5] == 0} >= {3, 4, 7, 8, 15, 16, 17}
    kinds = {(r[2], r[3] > 0, r[7], r[8]) for r in golden["rows"]}
    assert kinds == {(1, False, 0, 0), (1, False, 1, 0), (2, False, 0, 1), (2, False, 1, 1), (4, False, 0, 2),
                     (2, True, 0, 3), (2, True, 1, 3)}


F8C = dict(split=1, pv_split=1, f8=1)
SPLIT = dict(split=1, pv_split=0, f8=0)


def _shape(B, Hq, Hkv, nq, nk, window=0, has_part=1, causal=0, out_f32=0, **mode):
    return dict(B=B, Hq=Hq, Hkv=Hkv, nq=nq, nk=nk, window=window, causal=causal, has_part=has_part, out_f32=out_f32, **mode)


# 256 CUs, Hq 16 / Hkv 8 (64 queries per block): from the rules' comments and DESIGN.md section 4, not from the golden
LITERALS = [
    ("240 s full self-attention", _shape(1, 16, 8, 3000, 3000, **F8C),
     dict(n_blk=376, ksplit=2, split_from=256, grid=496, merge="tail", merge_grid=1920, kernel="attn_kh")),
    ("240 s full, split mode", _shape(1, 16, 8, 3000, 3000, **SPLIT),
     dict(n_blk=376, ksplit=2, split_from=256, grid=496, merge="tail", merge_grid=1920, kernel="attn2")),
    ("240 s sliding", _shape(1, 16, 8, 3000, 3000, window=128, **F8C),
     dict(n_blk=376, ksplit=1, split_from=0, grid=376, merge="none", merge_grid=0, kernel="attn2")),
    ("240 s cross", _shape(1, 16, 8, 3000, 512, **F8C),
     dict(n_blk=376, ksplit=1, split_from=0, grid=376, merge="none", merge_grid=0, kernel="attn2")),
    ("60 s full", _shape(1, 16, 8, 750, 750, **F8C),
     dict(n_blk=96, ksplit=2, split_from=0, grid=192, merge="uniform2", merge_grid=1500, kernel="attn2")),
    ("240 s, B = 8", _shape(8, 16, 8, 3000, 3000, **F8C),
     dict(n_blk=3008, ksplit=1, split_from=0, grid=3008, merge="none", merge_grid=0, kernel="attn_kh")),
    ("240 s, B = 8, split mode", _shape(8, 16, 8, 3000, 3000, **SPLIT),
     dict(n_blk=3008, ksplit=1, split_from=0, grid=3008, merge="none", merge_grid=0, kernel="attn2")),
    ("four-way split, 9 key tiles", _shape(1, 2, 1, 100, 566, **F8C),
     dict(n_blk=2, ksplit=4, split_from=0, grid=8, merge="uniform4", merge_grid=25, kernel="attn2")),
    ("four-way split, 10 key tiles", _shape(1, 2, 1, 100, 600, **F8C),
     dict(n_blk=2, ksplit=4, split_from=0, grid=8, merge="uniform4", merge_grid=25, kernel="attn2")),
]


@pytest.mark.parametrize("name,shape,want", LITERALS, ids=[l[0] for l in LITERALS])
def test_literal_plans(lib, golden, name, shape, want):
    c = capi()
    p = c.attn_plan(shape, lib=lib)
    assert {k: p[k] for k in want} == want and p["xcd_order"] == 1
    # the same case is in the golden, under the default policy, with the same answer
    si = golden["shapes"].index([shape[n] for n in c.ATTN_SHAPE_FIELDS])
    pi = golden["policies"].index([c.ATTN_POLICY_DEFAULT[n] for n in c.ATTN_POLICY_FIELDS])
    rows = [r for r in golden["rows"] if r[0] == si and r[1] == pi]
    assert rows and all(r[2:] == [p["ksplit"], p["split_from"], 1, p["n_blk"], p["grid"], c.ATTN_KERNELS.index(p["kernel"]),
                                  c.ATTN_MERGES.index(p["merge"]), p["merge_grid"]] for r in rows)


@pytest.mark.parametrize("nk,want", [(566, [3, 3, 3, 0]), (600, [3, 3, 3, 1])])
def test_four_way_split_parts(lib, nk, want):
    """test_attention_short_range_four_way_split's docstring: 9 / 10 key tiles in four parts, an empty last one."""
    got = [capi().attn_plan_tiles(nk, 0, False, 64, 64, part, 4, lib=lib) for part in range(4)]
    assert [n for _, n in got] == want
    assert [b for b, _ in got] == [0, 3, 6, 9]


def _cases(golden):
    """(shape, policy, plan) of every golden row, as dicts / lists."""
    c = capi()
    for si, pi, *plan in golden["rows"]:
        yield (dict(zip(c.ATTN_SHAPE_FIELDS, golden["shapes"][si])), dict(zip(c.ATTN_POLICY_FIELDS, golden["policies"][pi])),
               dict(zip(c.ATTN_PLAN_FIELDS, plan)))


def test_plan_field_constraints(lib, golden):
    c = capi()
    for s, pol, _ in _cases(golden):
        p = c.attn_plan(s, lib=lib, **pol)
        ctx = (s, pol, p)
        rep = s["Hq"] // s["Hkv"]
        qpb = 128 // rep
        rows = s["B"] * s["nq"] * s["Hq"]
        assert p["n_blk"] == s["B"] * s["Hkv"] * -(-s["nq"] // qpb), ctx
        assert p["ksplit"] in (1, 2, 4), ctx
        assert p["ksplit"] == 1 or s["has_part"], ctx
        assert p["split_from"] == 0 or (p["ksplit"] == 2 and 0 < p["split_from"] < p["n_blk"]), ctx
        assert p["split_from"] % 8 == 0 and p["grid"] % 8 == 0, ctx
        assert p["kernel"] == "attn2" or (s["split"] and s["pv_split"] and s["f8"]), ctx
        assert p["merge"] == ("none" if p["ksplit"] == 1 else "tail" if p["split_from"] else
                              "uniform2" if p["ksplit"] == 2 else "uniform4"), ctx
        if p["merge"] == "none":
            assert p["merge_grid"] == 0, ctx
        elif p["merge"] == "tail":  # 128 (query, head) rows per split block, 8 per workgroup
            assert p["merge_grid"] == (p["n_blk"] - p["split_from"]) * 16, ctx
        else:
            assert p["merge_grid"] == -(-rows // 8), ctx
        # the partials fit the workspace the engine allocates (attn_part_floats: 4 * rows * (128 + 2))
        assert p["ksplit"] * rows * 130 <= 4 * rows * 130, ctx


def _layouts(golden, max_grid):
    """The distinct (ksplit, split_from, n_blk, grid) of the golden, grids up to max_grid (the launch-index loops below
    run in Python)."""
    seen = set()
    for r in golden["rows"]:
        k = (r[2], r[3], r[5], r[6])
        if r[6] <= max_grid:
            seen.add(k)
    return sorted(seen)


def test_grid_covers_every_block_part_once(lib, golden):
    c = capi()
    layouts = _layouts(golden, 1024)
    assert len(layouts) >= 50
    assert {(k, f > 0) for k, f, _, _ in layouts} == {(1, False), (2, False), (4, False), (2, True)}
    for ksplit, split_from, n_blk, grid in layouts:
        want = sorted((b, p) for b in range(n_blk)
                      for p in range(1 if split_from and b < split_from else 2 if split_from else ksplit))
        for xcd in (0, 1):
            ctx = (ksplit, split_from, n_blk, grid, xcd)
            got, invalid = [], [0, 0]
            for x in range(grid):
                blk, part, parts, valid = c.attn_plan_block(ksplit, split_from, xcd, n_blk, x, lib=lib)
                if not valid:
                    invalid[1 if split_from and x >= split_from else 0] += 1
                    continue
                assert parts == (1 if split_from and blk < split_from else 2 if split_from else ksplit), (ctx, x)
                if xcd == 0:  # plain order: the map is the identity on valid indices
                    y = x - split_from if split_from and x >= split_from else x
                    base = split_from if split_from and x >= split_from else 0
                    assert (blk, part) == (base + y // parts, y % parts), (ctx, x)
                got.append((blk, part))
            assert sorted(got) == want, ctx
            assert max(invalid) <= 7 and len(got) + sum(invalid) == grid, (ctx, invalid)


def test_parts_tile_the_key_range(lib, golden):
    """For every block of a shape and every part count a plan can give it, the parts' key-tile ranges are ordered,
    disjoint and cover exactly the tiles a window / the causal mask leaves the block, an empty part having n = 0."""
    c = capi()
    shapes = {(128 // (s[1] // s[2]), s[3], s[4], s[5]) for s in golden["shapes"] if s[3] <= 4096}
    shapes |= {(64, 600, 1100, 0), (32, 150, 1100, 0), (64, 3000, 3000, 128)}
    checked = 0
    for qpb, nq, nk, window in sorted(shapes):
        n_qt = -(-nq // qpb)
        qts = sorted({0, 1, 2, n_qt // 2, n_qt - 2, n_qt - 1} & set(range(n_qt)))
        for causal in (False, True):
            for qt in qts:
                q0 = qt * qpb
                klo, khi = (max(0, q0 - window), min(nk, q0 + qpb + window)) if window else (0, nk)
                if causal:
                    khi = min(khi, q0 + qpb)
                lo, hi = klo // 64, max(klo // 64, -(-khi // 64))
                for parts in (1, 2, 4):
                    at = lo
                    for part in range(parts):
                        b, n = c.attn_plan_tiles(nk, window, causal, q0, qpb, part, parts, lib=lib)
                        assert n >= 0 and (n == 0 or b == at), (qpb, nq, nk, window, causal, qt, parts, part, b, n)
                        at += n
                    assert at == hi, (qpb, nq, nk, window, causal, qt, parts)
                    checked += 1
    assert checked > 1000


def test_entries_refuse_bad_arguments(lib):
    c = capi()
    ok = _shape(1, 2, 1, 600, 1100, **F8C)
    c.attn_plan(ok, lib=lib)
    for bad in (dict(ok, Hq=3, Hkv=2), dict(ok, Hq=8, Hkv=1), dict(ok, nq=0), dict(ok, Hkv=0)):
        with pytest.raises(ValueError):
            c.attn_plan(bad, lib=lib)
    for pol in (dict(ksplit_mode=5), dict(tail=2), dict(tail_min=1), dict(n_cu=0), dict(kh=2)):
        with pytest.raises(ValueError):
            c.attn_plan(ok, lib=lib, **pol)
    with pytest.raises(ValueError):
        c.attn_plan_tiles(1100, 0, False, 0, 64, 2, 2, lib=lib)
