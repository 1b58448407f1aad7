"""Filter/project cases at shapes where the two-pass kernels (hdk_amd/csrc/scan_project_fast.h) handle a block's tiles
in groups of four -- which needs more than 3 x grid tiles of 4096 rows in one fragment, so the GPU suite pins the grid
(Executor.prepare(grid=...)) -- with the expected rows in plain numpy.  The CPU suite checks the oracle against these
expectations (test_projection.py), the GPU suite checks the kernels against both (test_gpu_projection_groups.py).

Every query projects `rid`, the global row number: a row taken from the wrong tile or fragment shows by value."""
import numpy as np

from hdk_amd import _abi as A
from hdk_amd import result_set as rs
from hdk_amd.ir import Cmp, ColRef, JoinSpec, Lit, Proj, QueryUnit
from hdk_amd.storage import ArrowStorage

TILE_ROWS = 4096  # kProjFastBlock * kProjFastVR

# rows per fragment
LAYOUTS = {
    # 7 tiles + 1 row each (an odd row count: the pairs form ends on an unpaired row); with grid 2, block 1's group is
    # tiles 1, 3, 5, 7 and ends in the ragged tile
    "L1": [28673, 28673, 28673, 1],
    # 13 tiles + 3 rows, 10 tiles less one row: groups form at grids 1, 2 and 3; at grids 1 and 3 a group alternates tile
    # parity, so with `c` it holds dense and sparse tiles side by side
    "L2": [53251, 53251, 40959],
    # whole tiles only: a group's last tile is a full last tile
    "L3": [32768, 32768, 32768],
}

NULL_DOUBLE = np.frombuffer(np.int64(A.NULL_DOUBLE_BITS).tobytes(), dtype=np.float64)[0]

# name -> leaves (column, operator, literal), ANDed
FILTERS = {
    "a<37": [("a", "<", 37)],            # ~3.6 %: the *_pairs kernels, the sparse writing pass
    "a<600": [("a", "<", 600)],
    "a32<37": [("a32", "<", 37)],        # a 4-byte filter column: the lane-striped kernels
    "a32<600": [("a32", "<", 600)],
    "c<500": [("c", "<", 500)],          # ~50 % of the even tiles, ~3 % of the odd ones: dense pass, odd tiles through the strip
    "c<500&b>-100": [("c", "<", 500), ("b", ">", -100)],  # (the int32 leaf drops the pairs form)
    "a<-1": [("a", "<", -1)],            # no row
    "none": [],
}
TARGETS = ["rid", "a", "b", "s", "h", "d"]
JOIN_FILTERS = ["a<600", "a32<600"]
JOIN_TARGETS = ["rid", "v", "dim.w"]

_SENTINEL = {"a": A.NULL_BIGINT, "a32": A.NULL_INT, "c": A.NULL_BIGINT, "b": A.NULL_INT, "s": A.NULL_TINYINT,
             "h": A.NULL_SMALLINT}
_OPS = {"<": np.less, ">": np.greater, "<=": np.less_equal, ">=": np.greater_equal}


class Case:
    """One layout: the storage, its columns as whole arrays, the row position of every row inside its fragment."""

    def __init__(self, layout, frag_rows=None, columns=None, seed=None):
        self.layout = layout
        self.frag_rows = list(frag_rows if frag_rows is not None else LAYOUTS[layout])
        assert all(r == self.frag_rows[0] for r in self.frag_rows[:-1]) and self.frag_rows[-1] <= self.frag_rows[0]
        n = self.n = int(sum(self.frag_rows))
        rng = np.random.default_rng(seed if seed is not None else 4100 + sorted(LAYOUTS).index(layout))
        self.frag_of = np.repeat(np.arange(len(self.frag_rows)), self.frag_rows)
        self.frag_start = np.concatenate([[0], np.cumsum(self.frag_rows)])[:-1].astype(np.int64)
        self.pos = np.arange(n, dtype=np.int64) - self.frag_start[self.frag_of]
        # launch-global index of the first tile of each fragment: tiles cumulated over the fragments
        tiles = [(r + TILE_ROWS - 1) // TILE_ROWS for r in self.frag_rows]
        self.frag_tile_base = np.concatenate([[0], np.cumsum(tiles)])[:-1].astype(np.int64)
        self.num_tiles = int(sum(tiles))
        cols = {"rid": np.arange(n, dtype=np.int64)}
        a = rng.integers(0, 1000, n).astype(np.int64)
        a_null = rng.random(n) < 0.03
        cols["a"] = np.where(a_null, A.NULL_BIGINT, a)
        cols["b"] = rng.integers(-500, 500, n).astype(np.int32)
        cols["b"][rng.random(n) < 0.05] = A.NULL_INT
        if columns is None or "a32" in columns:
            cols["a32"] = np.where(a_null, A.NULL_INT, a).astype(np.int32)
            cols["c"] = np.where(a_null, A.NULL_BIGINT, a + 470 * ((self.pos // TILE_ROWS) & 1))
            cols["s"] = rng.integers(-100, 100, n).astype(np.int8)
            cols["s"][rng.random(n) < 0.05] = A.NULL_TINYINT
            cols["h"] = rng.integers(-30000, 30000, n).astype(np.int16)
            cols["h"][rng.random(n) < 0.05] = A.NULL_SMALLINT
            cols["d"] = rng.normal(size=n)
            cols["d"][rng.random(n) < 0.05] = NULL_DOUBLE
            # the join: 1000 unique odd keys 5..2003; fk hits one, misses (even, or out of range), or is NULL
            nd = 1000
            self.dim_key = rng.permutation(nd).astype(np.int64) * 2 + 5
            self.dim_w = rng.integers(-50, 50, nd).astype(np.int32)
            self.dim_w[rng.random(nd) < 0.05] = A.NULL_INT
            cols["fk"] = rng.integers(0, 2 * nd + 20, n).astype(np.int64)
            cols["fk"][rng.random(n) < 0.03] = A.NULL_BIGINT
            cols["v"] = rng.integers(0, 10**6, n).astype(np.int64)
        if columns is not None:
            cols = {k: v for k, v in cols.items() if k in columns}
        self.cols = cols
        self.st = ArrowStorage()
        self.st.import_numpy("t", cols, fragment_size=self.frag_rows[0])
        assert self.st.get("t").frag_rows == self.frag_rows
        if "fk" in cols:
            self.st.import_numpy("dim", {"key": self.dim_key, "w": self.dim_w})

    def tile_of_rid(self, rid):
        """launch-global tile index of global rows `rid`"""
        f = self.frag_of[rid]
        return self.frag_tile_base[f] + (rid - self.frag_start[f]) // TILE_ROWS


def query(filter_name, columnar, targets=None, scan_limit=None, join=False):
    quals = [Cmp(ColRef(c), op, Lit(v)) for c, op, v in FILTERS[filter_name]]
    targets = targets or (JOIN_TARGETS if join else TARGETS)
    proj = [Proj(ColRef(*reversed(t.split("."))), t.replace(".", "_")) for t in targets]
    return QueryUnit("t", joins=[JoinSpec("dim", ColRef("fk"), "key")] if join else [], quals=quals, targets=proj,
                     output_columnar=columnar, scan_limit=scan_limit)


def keep_mask(case, filter_name, join=False):
    """A leaf keeps a row iff the column is not its sentinel and the comparison holds; an inner join keeps a row iff its
    key is not NULL and has a partner."""
    keep = np.ones(case.n, dtype=bool)
    for c, op, v in FILTERS[filter_name]:
        col = case.cols[c]
        keep &= (col != _SENTINEL[c]) & _OPS[op](col.astype(np.int64), v)
    if join:
        fk = case.cols["fk"]
        keep &= (fk != A.NULL_BIGINT) & np.isin(fk, case.dim_key)
    return keep


def expected_rows(case, filter_name, targets=None, join=False):
    """The sorted (row position inside the fragment, targets...) matrix: column values sign-extended to int64, doubles
    as their bit patterns."""
    keep = keep_mask(case, filter_name, join)
    out = [case.pos[keep]]
    for t in targets or (JOIN_TARGETS if join else TARGETS):
        if t == "dim.w":
            by_key = np.full(int(case.dim_key.max()) + 1, 0, dtype=np.int64)
            by_key[case.dim_key] = case.dim_w
            out.append(by_key[case.cols["fk"][keep]])
        else:
            col = case.cols[t][keep]
            out.append(col.view(np.int64) if col.dtype.kind == "f" else col.astype(np.int64))
    return sort_rows(np.stack(out, axis=1))


def sort_rows(m):
    return m[np.lexsort(m.T[::-1])]


def buffer_rows(cp, buf, n, sort=True):
    """(row position, targets...) of the first n rows of a projection buffer, in buffer order or sorted"""
    pos, cols = rs.projection_arrays(cp, buf, n)
    m = np.stack([pos] + cols, axis=1) if len(pos) else np.zeros((0, 1 + len(cols)), dtype=np.int64)
    return sort_rows(m) if sort else m
