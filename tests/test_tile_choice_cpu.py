"""What `ops.gemm(tile=0)` picks, without a device: the Python-side tile constants against the `switch` statements of
csrc/gemm.hip (parsed as text, the way tests/test_abi.py reads include/avsd.h), the two static rules (_heuristic_tile /
_heuristic_tile_x2) over a grid that reaches every one of their branches, the repair of a sub-pixel upsample convolution's pick
(_subpix_tile: the column tile must divide cout, gemm.hip launch2), and the committed table asva_amd/tiles_gfx950.json.
Nothing here loads the library; tests/test_tile_choice_gpu.py runs the picks."""
import json
import os
import re

import pytest

from asva_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_ints():
    src = open(os.path.join(ROOT, "include", "avsd.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(AVSD_GEMM_\w+)\s+(\d+)\b", src)}


def _dispatcher(name):
    """{tile id: (BM, BN)} of the `switch (tile)` in the DEFINITION of `name` (a declaration ends in ';' and has no body)"""
    src = open(os.path.join(ROOT, "asva_amd", "csrc", "gemm.hip")).read()
    m = re.search(r"\bint\s+" + name + r"\(const avsd_gemm_desc& d, int tile, hipStream_t s\)\s*\{\s*switch \(tile\) \{(.*?)\bdefault:", src, re.S)
    assert m, f"{name}: definition not found in csrc/gemm.hip"
    body = re.sub(r"//[^\n]*", "", m.group(1))
    ints = _header_ints()
    cases = re.findall(r"case\s+(\w+)\s*:\s*return\s+launch2?<\s*(\d+)\s*,\s*(\d+)\s*,", body)
    assert len(cases) == len(re.findall(r"\bcase\b", body)), f"{name}: a case label this test cannot read"
    return {(int(t) if t.isdigit() else ints[t]): (int(bm), int(bn)) for t, bm, bn in cases}


@pytest.fixture(scope="module")
def built():
    return {"one": _dispatcher("dispatch_tile"), "x2": _dispatcher("dispatch_tile_x2"),
            "subpix": _dispatcher("avsd_gemm_dispatch_subpix"), "subpix_x2": _dispatcher("avsd_gemm_dispatch_x2_subpix")}


# ---- a. the hand-copied constants ---------------------------------------------------------------------------------------
def test_python_tile_constants_match_the_c_dispatchers(built):
    assert 38 in built["one"] and _header_ints()["AVSD_GEMM_TILE_256x160_8W"] == 38
    assert len(built["one"]) >= 19 and len(built["x2"]) == 8
    for t, bn in ops.TILE_BN.items():
        seen = [d[t][1] for d in built.values() if t in d]
        assert seen, f"TILE_BN lists tile {t}, which no dispatcher builds"
        assert set(seen) == {bn}, f"TILE_BN[{t}] = {bn}, gemm.hip builds BN {sorted(set(seen))}"
    assert set(ops.SUBPIX_TILES) == set(built["subpix"])
    assert set(ops.SUBPIX_X2_TILES) == set(built["subpix_x2"])
    # a tile keeps its block in every dispatcher that builds it, and every sub-pixel tile has a width on the Python side
    for t in set(built["subpix"]) | set(built["subpix_x2"]):
        assert t in ops.TILE_BN
    for t in built["subpix"]:
        assert built["subpix"][t] == built["one"][t]
    for t in built["subpix_x2"]:
        assert built["subpix_x2"][t] == built["x2"][t]
    for name, dset in (("TILE_CANDIDATES", "one"), ("SPLITK_CANDIDATES", "one"), ("X2_TILE_CANDIDATES", "x2"), ("X2_SPLITK_CANDIDATES", "x2")):
        missing = sorted({t for t, _ in getattr(ops, name)} - set(built[dset]))
        assert not missing, f"ops.{name} offers tiles {missing} that gemm.hip does not build"
    # split-K candidates lie in the id range avsd_gemm_bf16 lets split (4 .. AVSD_GEMM_MAX_TILE[_X2], and 38 in one pass)
    ints = _header_ints()
    assert all(4 <= t <= ints["AVSD_GEMM_MAX_TILE"] or t == 38 for t, _ in ops.SPLITK_CANDIDATES)
    assert all(4 <= t <= ints["AVSD_GEMM_MAX_TILE_X2"] for t, _ in ops.X2_SPLITK_CANDIDATES)
    assert ops.ASM_TILES == tuple(range(ints["AVSD_GEMM_TILE_ASM_FIRST"], ints["AVSD_GEMM_TILE_ASM_LAST"] + 1))
    assert ops.NSTREAM_TILE == ints["AVSD_GEMM_TILE_NSTREAM"]


# ---- b. the two rules ---------------------------------------------------------------------------------------------------
GRID_M = (8, 77, 256, 1280, 3584, 5760, 7168, 14336, 28672, 98304)
GRID_N = (4, 64, 132, 320, 512, 640, 1280, 5120)
GRID_K = (64, 200, 256, 512, 1024, 4096, 23040)
# one (M, N, K) per `return` of each rule (geglu off, split-K allowed): -> (tile, split_k)
BRANCH_POINTS = {
    "one": {(14336, 512, 1024): (20, 1), (14336, 512, 256): (14, 1), (7168, 512, 512): (30, 1), (7168, 512, 256): (11, 1),
            (5760, 320, 1024): (24, 1), (5760, 320, 256): (12, 1), (3584, 320, 512): (25, 1), (1280, 320, 256): (13, 1),
            (1280, 320, 512): (25, 2), (256, 320, 4096): (25, 8)},
    "x2": {(14336, 320, 512): (34, 1), (7168, 512, 256): (11, 1), (5760, 320, 512): (24, 1), (3584, 320, 512): (25, 1),
           (1280, 320, 256): (13, 1), (1280, 320, 512): (25, 2), (256, 320, 4096): (25, 8)},
}


def _rule(which):
    return ops._heuristic_tile_x2 if which == "x2" else ops._heuristic_tile


@pytest.mark.parametrize("which", ["one", "x2"])
def test_rules_return_built_tiles_and_legal_splits(built, which):
    rule, reached = _rule(which), set()
    for M in GRID_M:
        for N in GRID_N:
            for K in GRID_K:
                for geglu in (False, True):
                    for splitk_ok in (False, True):
                        tile, sk = rule(M, N, K, geglu, splitk_ok)
                        at = (which, M, N, K, geglu, splitk_ok)
                        assert tile in built[which], (at, tile)
                        nk = (K + 63) // 64
                        if geglu or not splitk_ok:
                            assert sk == 1, (at, sk)
                        else:
                            # avsd_gemm_bf16: split_k <= ceil(K / 64); gemm2_kernel gives slice s the K tiles [s * per, (s + 1) * per), per = ceil(nk / sk)
                            assert 1 <= sk <= nk and (sk - 1) * -(-nk // sk) < nk, (at, sk)
                            assert sk == 1 or tile in {t for t, _ in (ops.X2_SPLITK_CANDIDATES if which == "x2" else ops.SPLITK_CANDIDATES)}, (at, tile, sk)
                        reached.add((tile, min(sk, 2)))
    # every `return` of the rule: its tile, and for the last one a split > 1
    returns = {(20, 1), (14, 1), (30, 1), (11, 1), (24, 1), (12, 1), (25, 1), (13, 1), (25, 2)} if which == "one" else \
              {(34, 1), (11, 1), (24, 1), (25, 1), (13, 1), (25, 2)}
    assert reached == returns, sorted(reached ^ returns)


@pytest.mark.parametrize("which", ["one", "x2"])
def test_rule_branch_points_land_where_stated(which):
    """the points tests/test_tile_choice_gpu.py launches, one per branch: all on the grid above"""
    for (M, N, K), want in BRANCH_POINTS[which].items():
        assert M in GRID_M and N in GRID_N and K in GRID_K
        assert _rule(which)(M, N, K, False, True) == want, (which, M, N, K)
    assert {t for t, _ in BRANCH_POINTS[which].values()} == ({20, 14, 30, 11, 24, 12, 25, 13} if which == "one" else {34, 11, 24, 25, 13})
    assert {sk for _, sk in BRANCH_POINTS[which].values()} >= {1, 2, 8}


# ---- c. the sub-pixel upsample convolution's pick -----------------------------------------------------------------------
def _parent_subpix(t, cout, x2):
    """the rule this project shipped before _subpix_tile, and whether its answer could launch"""
    ok_tiles = ops.SUBPIX_X2_TILES if x2 else ops.SUBPIX_TILES
    if t not in ok_tiles or cout % ops.TILE_BN[t]:
        t = {14: 20, 12: 24}.get(t, 11)
    return t, (t in ok_tiles and cout % ops.TILE_BN[t] == 0)


def _subpix_pick(M, cin, cout, x2):
    t, sk = _rule("x2" if x2 else "one")(M, 4 * cout, 4 * cin, False, True)
    return t, sk, ops._subpix_tile(t, cout, x2)


@pytest.mark.parametrize("x2", [False, True], ids=["one_pass", "x2"])
def test_subpixel_pick_is_always_legal_and_shipped_picks_do_not_move(x2):
    ok_tiles = ops.SUBPIX_X2_TILES if x2 else ops.SUBPIX_TILES
    illegal, moved, parent_illegal = [], [], 0
    for cout in range(64, 2048 + 1, 64):
        for cin in (64, 256, 1280):
            for M in GRID_M:
                t, sk, got = _subpix_pick(M, cin, cout, x2)
                if got not in ok_tiles or cout % ops.TILE_BN[got]:
                    illegal.append((cout, cin, M, t, got))
                old, old_ok = _parent_subpix(t, cout, x2)
                parent_illegal += not old_ok
                if old_ok and got != old:
                    moved.append((cout, cin, M, t, old, got))
                assert ops.TILE_BN[got] <= max(ops.TILE_BN[t], 64)
    assert not illegal, f"(cout, cin, M, rule tile, final tile) the C dispatcher refuses: {illegal}"
    assert not moved, f"(cout, cin, M, rule tile, parent's tile, new tile): a legal pick moved: {moved}"
    assert parent_illegal > 0          # (the sweep covers what the earlier rule got wrong: cout = 320 / 448 / ... at large M)


# upsampler convolutions of the shipped networks, (n_img, hs, ws, cin = cout): the SD1.5-shaped UNet at 12 x 256 x 256 with CFG
# (configurations 1-3: 24 images, 32 x 32 latents) and at 24 x 512 x 512 (configuration 4: 48 images, 64 x 64 latents), and the VAE
# decoder's three upsamplers on 32 x 32 and 64 x 64 latents, 1 / 12 / 24 frames per decode chunk
SHIPPED_UPSAMPLERS = [(n, s, s, c) for n, side in ((24, 32), (48, 64)) for s, c in ((side // 8, 1280), (side // 4, 1280), (side // 2, 640))] + \
                     [(n, s, s, c) for n in (1, 12, 24) for side in (32, 64) for s, c in ((side, 512), (2 * side, 512), (4 * side, 256))]


@pytest.mark.parametrize("x2", [False, True], ids=["one_pass", "x2"])
@pytest.mark.parametrize("n_img,hs,ws,c", SHIPPED_UPSAMPLERS)
def test_shipped_upsamplers_keep_their_tiles(n_img, hs, ws, c, x2):
    assert not any(k[0] == ops.CONV3 and k[6] == 2 for k in ops.tile_cache() if k[0] != "batched")      # the rule places every one of them
    t, sk, got = _subpix_pick(n_img * hs * ws, c, c, x2)
    old, old_ok = _parent_subpix(t, c, x2)
    assert old_ok and got == old, (n_img, hs, ws, c, t, old, got)


def test_subpix_tile_is_total_and_keeps_legal_picks():
    """any tile id the table could name (built here or not), any cout the gate admits"""
    for x2 in (False, True):
        ok_tiles = ops.SUBPIX_X2_TILES if x2 else ops.SUBPIX_TILES
        for cout in range(64, 2048 + 1, 64):
            for t in list(range(0, 71)):
                got = ops._subpix_tile(t, cout, x2)
                assert got in ok_tiles and cout % ops.TILE_BN[got] == 0, (x2, cout, t, got)
                if t in ok_tiles and cout % ops.TILE_BN[t] == 0:
                    assert got == t
                assert ops.TILE_BN[got] <= max(ops.TILE_BN.get(t, 128), 64)     # never a wider column tile than the pick
    for bad in (0, 32, 96, -64):
        with pytest.raises(ValueError):
            ops._subpix_tile(11, bad, False)
    # the cases the earlier rule sent to a 128-wide tile whatever cout was
    assert ops._subpix_tile(14, 320, False) == 24 and ops._subpix_tile(30, 320, False) == 24 and ops._subpix_tile(11, 192, True) == 24
    assert ops._subpix_tile(14, 640, False) == 20 and ops._subpix_tile(12, 320, False) == 24 and ops._subpix_tile(11, 64, True) == 24


# ---- d. the committed table ---------------------------------------------------------------------------------------------
def _table():
    with open(ops.DEFAULT_TILE_TABLE) as f:
        return [(tuple(k), tuple(v)) for k, v in json.load(f)]


def test_committed_table_names_only_tiles_its_key_can_run(built):
    table = _table()
    assert len(table) > 1000
    asm_x2 = {t for t, _ in ops.ASM_X2_CANDIDATES + ops.ASM_X2_SPLITK_CANDIDATES}
    resident = set(ops.CONV3R_TILES) | set(ops.CONV3R2D_TILES)
    bad = []
    for key, (tile, sk) in table:
        if key[0] == "batched":                      # gemm_batched: ("batched", B, M, N, K, flags), PLAIN, no split
            _, B, M, N, K, flags = key
            if tile not in built["x2" if flags & ops.X2 else "one"] or sk != 1:
                bad.append((key, tile, sk, "batched: not an LDS-direct / register-staged tile of this precision"))
            continue
        mode, M, N, K, flags, stride, ups, pad, key_master = key[:9]
        x2 = bool(flags & ops.X2)
        a2 = "a2" in key
        assert mode in (ops.PLAIN, ops.TMIX, ops.CONV3) and len(key) in (9, 11, 13)
        assert (len(key) >= 11 and isinstance(key[9], int)) == (mode == ops.CONV3 and not x2), key       # one-pass convolutions carry (hs, ws)
        why = None
        if sk < 1 or sk > (K + 63) // 64 or (sk > 1 and flags & ops.GEGLU):
            why = "split_k outside 1 .. ceil(K / 64), or with GEGLU"
        elif mode == ops.CONV3 and ups == 2:
            if tile not in (ops.SUBPIX_X2_TILES if x2 else ops.SUBPIX_TILES) or N % 4 or (N // 4) % ops.TILE_BN[tile]:
                why = "ups = 2: not a sub-pixel tile whose BN divides N / 4"
        elif tile in ops.ASM_TILES:
            if mode not in (ops.PLAIN, ops.TMIX) or K % 64 or (mode == ops.TMIX and tile == 60) or (x2 and tile not in asm_x2):
                why = "asm tile outside PLAIN / TMIX with K % 64 == 0 (TMIX: 61..67; split precision: 63..66)"
        elif tile in resident or 40 <= tile <= 54:
            if tile not in resident or mode != ops.CONV3 or stride != 1 or ups != 0 or x2:
                why = "resident convolution tile outside one-pass CONV3 with stride 1, ups 0"
        elif tile not in built["x2" if x2 else "one"]:
            why = "not built by dispatch_tile" + ("_x2" if x2 else "")
        elif sk > 1 and tile < 4:
            why = "split_k on a register-staged tile"
        if a2 and tile not in resident:
            why = "two-source convolution on a tile that reads one source"
        if why:
            bad.append((key, tile, sk, why))
    assert not bad, bad
    assert sum(1 for k, _ in table if k[0] == ops.CONV3 and k[6] == 2) == 0      # (today the rule places every sub-pixel convolution)
