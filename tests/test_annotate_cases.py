"""annotate_cases.py checked on the CPU: the definition-based reference equals
the numpy transcription of annotate.hip's closed forms on every planted and
random case (which pins the identities, the zero-width term included), the
planted cases place what their docstrings claim against the kernel's tile and
window constants, and the header, the binding, the library and the CLI carry
the new surface."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import annotate_cases as ac
from tests.annotate_cases import T, W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED = {c["name"]: c for c in ac.planted_cases()}
ANNOT_SYMBOLS = ("lime_annotate", "lime_annot_size", "lime_annot_fill_host",
                 "lime_annot_device_arrays", "lime_annot_totals", "lime_annot_format_bed",
                 "lime_annot_destroy")


@functools.lru_cache(maxsize=None)
def _ref(name):
    c = PLANTED[name]
    return ac.annotate_ref(c["A"], c["B"], c["lens"])


def _same(x, y):
    return all(np.array_equal(np.asarray(a, np.int64), np.asarray(b, np.int64))
               for a, b in zip(x, y))


# ---------------------------------------------------------------- identities
@pytest.mark.parametrize("name", sorted(PLANTED))
def test_closed_forms_equal_the_definition(name):
    c = PLANTED[name]
    assert _same(ac.closed_forms(c["A"], c["B"], c["lens"]), _ref(name))


@pytest.mark.parametrize("seed", range(6))
def test_closed_forms_on_random_heavy_ties(seed):
    # 3000 x 3000 rows from ~2,100 coordinates (the mask reference), 15 % and
    # then 50 % zero-width rows on both sides
    c = ac.random_pair(4000 + 2 * seed, 3000, 40)
    if seed >= 3:
        for side in ("A", "B"):
            z = np.random.default_rng(seed).random(3000) < 0.5
            c[side][2][z] = c[side][1][z]
    ref = ac.annotate_ref(c["A"], c["B"], c["lens"])
    assert _same(ac.closed_forms(c["A"], c["B"], c["lens"]), ref)
    zw = c["A"][1] == c["A"][2]
    assert zw.sum() > 300 and ref[0][zw].max() > 0 and (ref[1][zw] == 0).all()


def test_oracle_route_equals_the_mask():
    c = ac.random_pair(4100, 3000, 40)
    A, B = ac._cols(c["A"]), ac._cols(c["B"])
    assert _same(ac._hits_by_oracle(A, B, c["lens"]), ac._hits_by_mask(A, B))


# -------------------------------------------------- what the planted cases claim
@pytest.mark.parametrize("case,want", ac.edge_cases() + ac.contig_cases(),
                         ids=lambda v: v["name"] if isinstance(v, dict) else "")
def test_edge_semantics(case, want):
    assert _same(_ref(case["name"]), want)


def test_degenerate_shapes():
    assert [len(v) for v in _ref("empty_a")] == [0, 0, 0]
    assert [v.tolist() for v in _ref("empty_b")] == [[0, 0, 0]] * 3
    assert [len(v) for v in _ref("both_empty")] == [0, 0, 0]
    assert [v.tolist() for v in _ref("one_each")] == [[1], [4], [4]]


def test_wide_counts_pass_16_and_32_bits():
    h, c, o = _ref("wide")
    assert h.tolist() == [70_000] and h[0] > 2 ** 16
    assert c.tolist() == [70_000]
    assert o.tolist() == [70_000 * 70_000] and o[0] > 2 ** 32


def test_long_b_is_found_by_four_tiles():
    c = PLANTED["long_b_over_tiles"]
    assert len(c["A"][0]) == 3 * T + 5
    win = ac.tile_windows(c["A"], c["B"], c["lens"])
    assert len(win) == 4 and win[:, 0].tolist() == [1, 0, 0, 1]  # its start: tile 0's window
    h, cov, o = _ref("long_b_over_tiles")
    under = c["A"][1] >= 5
    assert h[~under].tolist() == [0, 0] and (h[under] >= 1).all() and h.max() == 2
    assert (cov[under] == 1).all() and (o[under] == h[under]).all()


def test_long_first_row_leaves_its_window():
    c = PLANTED["long_first_row"]
    order = np.lexsort((c["A"][2], c["A"][1]))
    first = order[T]  # the first row of tile 1
    s, e = int(c["A"][1][first]), int(c["A"][2][first])
    assert (s, e) == (T, 12 * T)
    # tile 1's window of starts ends where A's last start falls; the row's
    # end lies beyond, among B rows
    last_start = int(c["A"][1].max())
    bs = np.sort(c["B"][1])
    assert np.searchsorted(bs, e) - np.searchsorted(bs, last_start) > W
    assert _ref("long_first_row")[0][first] > W


@pytest.mark.parametrize("n", ac.TILE_ROWS)
def test_tile_sized_row_counts(n):
    c = PLANTED[f"tile_sized_{n}"]
    assert len(c["A"][0]) == n and n in (T - 1, T, T + 1, 2 * T + 1, 3 * T - 1)
    assert len(np.unique(c["B"][1])) <= 40 and _ref(c["name"])[0].max() > 50


@pytest.mark.parametrize("m", ac.WINDOW_ROWS)
def test_window_cases_hold_exactly_m(m):
    c = PLANTED[f"window_{m}"]
    win = ac.tile_windows(c["A"], c["B"], c["lens"])
    assert win[0].tolist() == [m, m, m] and m in (W - 1, W, W + 1)
    assert (win[1] < 100).all()  # the next tile is staged whatever tile 0 did


def test_empty_window_cases():
    for name in ("b_before_a", "b_after_a"):
        c = PLANTED[name]
        assert (ac.tile_windows(c["A"], c["B"], c["lens"])[:, 0] == 0).all(), name
        assert (_ref(name)[0] == 0).all()
    c = PLANTED["b_in_gap"]
    win = ac.tile_windows(c["A"], c["B"], c["lens"])
    assert win[:, 0].tolist() == [0, 100, 0] and (_ref("b_in_gap")[0] == 0).all()


def test_format_annot():
    c, want = ac.contig_cases()[1]
    assert ac.format_annot(["x", "y", "z"], c["A"], want) == \
        b"x\t1\t4\t0\t0\t0\ny\t0\t5\t1\t3\t3\ny\t6\t7\t0\t0\t0\n"


def test_constants_match_the_kernel():
    src = open(os.path.join(ROOT, "lime_amd", "csrc", "annotate.hip")).read()
    anb = int(re.search(r"constexpr int ANB = (\d+);", src).group(1))
    items = int(re.search(r"constexpr int AN_ITEMS = (\d+);", src).group(1))
    w = int(re.search(r"constexpr int AN_W = (\d+);", src).group(1))
    assert "AN_TILE = ANB * AN_ITEMS" in src and anb * items == T and w == W
    assert "<= AN_W" in src  # a window of exactly W entries is staged


# ---------------------------------------------------- header, library, CLI
def test_header_declares_and_library_exports_annotate():
    import ctypes
    from lime_amd import _ffi
    header = open(os.path.join(ROOT, "include", "lime_amd.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    assert sorted(set(re.findall(r"\b(lime_annot\w*)\(", header))) == sorted(ANNOT_SYMBOLS)
    for name in ANNOT_SYMBOLS:
        assert name in _ffi.SIGNATURES, name
        assert getattr(lib, name) is not None, name
    assert re.search(r"#define LIME_ABI_VERSION 6\b", header)


def test_cli_lists_annotate():
    r = subprocess.run([os.path.join(ROOT, "bin", "lime-submit")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0
    assert re.search(r"^\s*annotate : ", r.stdout, re.M)
