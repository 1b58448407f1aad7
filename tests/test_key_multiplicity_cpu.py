"""The host side of joining against a device result (hdk_hip_key_multiplicity, storage.DeviceTable.key_multiplicity,
Executor.compile / drop_registered, a JoinSpec whose inner table is a QueryUnit): the numpy evaluator of the call's contract
(tests/multiplicity_expect.py) against the planner's own count over host fragments, the C ABI's argument checks, which come
back before any device is touched, the workspace arithmetic, the plans a DeviceTable with its number compiles to -- byte for
byte those of a host table with the same values -- and the refusals.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from hdk_amd import _abi as A
from hdk_amd import storage as S
from hdk_amd._lib import lib
from hdk_amd.executor import Executor
from hdk_amd.ir import Agg, BinOp, ColRef, JoinSpec, KeyRef, Proj, QueryMustRunOnCpu, QueryUnit, Type
from hdk_amd.plan import _inner_max_matches, compile_query, join_key_shape, multiplicity_key

import multiplicity_expect as M
from multiplicity_expect import NULL_I64

I8, I8N = Type("int", 8, False), Type("int", 8, True)
DATE_S = Type("date", 8, True, unit="s")
DAY = 86400


def inner_columns(n=600, seed=11):
    """u: unique; k: 0..39 with NULLs; d: seconds over 30 days, several rows a day, negative days and NULLs; a, b, c:
    components of composite keys with NULLs, the most frequent (a, b) pair carrying a NULL in c"""
    rng = np.random.default_rng(seed)
    u = rng.permutation(n).astype(np.int64) + 100
    k = rng.integers(0, 40, n).astype(np.int64)
    k[rng.random(n) < 0.1] = NULL_I64
    d = (rng.integers(-10, 20, n) * DAY + rng.integers(0, DAY, n)).astype(np.int64)
    d[rng.random(n) < 0.1] = NULL_I64
    a = rng.integers(0, 6, n).astype(np.int64)
    b = rng.integers(-3, 3, n).astype(np.int64)
    c = rng.integers(0, 2, n).astype(np.int64)
    a[rng.random(n) < 0.05] = NULL_I64
    b[rng.random(n) < 0.05] = NULL_I64
    a[:50], b[:50], c[:50] = 7, 7, NULL_I64
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    return {"u": u, "k": k, "d": d, "a": a, "b": b, "c": c, "v": v}


TYPES = {"u": I8, "k": I8N, "d": DATE_S, "a": I8N, "b": I8N, "c": I8N, "v": I8}
ORDER = list(TYPES)


def host_inner(frag=256):
    st = S.ArrowStorage()
    return st, st.import_numpy("dimr", inner_columns(), fragment_size=frag, types=TYPES)


def evaluate(table, cols_data, spec):
    """the evaluator asked as the executor asks the device: keys and route from plan.join_key_shape"""
    shape = join_key_shape(table, spec)
    keys = []
    for c in shape.cols:
        stt = table.columns[c].table_stats()
        keys.append(M.key(ORDER.index(c), True, int(NULL_I64), int(stt.min), int(stt.max)))
    got = M.expect([cols_data[c] for c in ORDER], len(cols_data["u"]), keys, shape.entry_count, shape.bucket, shape.nulls_match)
    return shape, got


SPECS = {
    "unique": JoinSpec("dimr", ColRef("fk"), "u"),
    "many": JoinSpec("dimr", ColRef("fk"), "k"),
    "many_null_safe": JoinSpec("dimr", ColRef("fk"), "k", null_safe=True),
    "date": JoinSpec("dimr", ColRef("fd"), "d"),
    "date_null_safe": JoinSpec("dimr", ColRef("fd"), "d", null_safe=True),
    "two": JoinSpec("dimr", [ColRef("fa"), ColRef("fb")], ["a", "b"]),
    "three": JoinSpec("dimr", [ColRef("fa"), ColRef("fb"), ColRef("fc")], ["a", "b", "c"]),
}


# ---- the evaluator against the planner's count over host fragments --------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SPECS))
def test_evaluator_agrees_with_the_planners_count(name):
    _, t = host_inner()
    data = inner_columns()
    shape, got = evaluate(t, data, SPECS[name])
    want = _inner_max_matches(t, shape.cols, shape.nulls_match, shape.bucket)
    assert (got[0] or 1) == want, (name, got, want)
    assert got[3] == 0  # (fresh statistics: nothing outside the range)
    if name == "unique":
        assert got[:3] == (1, 600, 600) and not shape.keyed and shape.entry_count == 600
    if name == "date":
        assert shape.bucket == DAY and got[0] > 1 and got[1] <= 30
    if name == "many_null_safe":
        nulls = int((data["k"] == NULL_I64).sum())
        assert got[2] == 600 and got[0] >= nulls > 0
    if name == "three":
        assert shape.keyed and shape.entry_count == 0
        assert got[0] < 50  # (the 50 rows of (7, 7, NULL) are skipped)
    if name == "two":
        assert got[0] == 50


def test_evaluator_rules():
    k = M.key(0, True, int(NULL_I64), 10, 20)
    col = [np.array([10, 20, 9, 21, int(NULL_I64), 15, 15], dtype=np.int64)]
    assert M.perfect(col, 7, k, 11) == (2, 3, 4, 2)
    assert M.perfect(col, 7, k, 12, nulls_match=True) == (2, 4, 5, 2)
    assert M.perfect(col, 7, k, 6) == (2, 2, 3, 3)  # (slot 10 of key 20 lies outside a table of 6)
    assert M.perfect(col, 7, M.key(0, False, int(NULL_I64), 10, 20), 11) == (2, 3, 4, 3)  # (not nullable: the word is a value)
    assert M.perfect(col, 0, k, 11) == (0, 0, 0, 0)
    two = [np.array([1, 1, 1, 2], dtype=np.int64), np.array([5, 5, int(NULL_I64), 5], dtype=np.int64)]
    assert M.sorted_route(two, 4, [M.key(0), M.key(1)]) == (2, 2, 3, 0)
    assert M.sorted_route(two, 4, [M.key(0)]) == (3, 2, 4, 0)


# ---- the C ABI: argument errors before any device, workspace arithmetic -------------------------------------------------
def _keys(*cols, mn=0, mx=99):
    arr = (A.MultiplicityKey * max(len(cols), 1))()
    for i, c in enumerate(cols):
        arr[i] = A.MultiplicityKey(c, 1, (C.c_uint8 * 3)(), int(NULL_I64), mn, mx, mx + 1)
    return arr


def test_invalid_arguments_come_back_before_any_device():
    L = lib()
    # (never dereferenced: every check comes first) cols 3 x 100 words at 4096, the record at 1 << 20

    def call(cols=4096, cap=100, nc=3, n=100, keys=_keys(1), nk=1, entries=100, bucket=1, flags=0, rec=1 << 20, ws=None, ws_bytes=0,
             device=0):
        st = L.hdk_hip_key_multiplicity(cols, cap, nc, n, keys, nk, entries, bucket, flags, rec, ws, ws_bytes, device, None)
        return st, (L.hdk_hip_last_error() or b"").decode()

    for kw in ({"cols": None}, {"keys": None}, {"rec": None}):
        st, msg = call(**kw)
        assert st == A.ERR_INVALID_ARG and "NULL" in msg, kw
    for nk in (0, 4, -1):
        st, msg = call(nk=nk, keys=_keys(0, 1, 2, 0), entries=0)
        assert st == A.ERR_INVALID_ARG and "num_keys" in msg, nk
    for keys in (_keys(3), _keys(-1)):
        st, msg = call(keys=keys)
        assert st == A.ERR_INVALID_ARG and "names column" in msg
    st, msg = call(keys=_keys(0, 3), nk=2, entries=0)
    assert st == A.ERR_INVALID_ARG and "names column" in msg
    st, msg = call(n=2**32, cap=2**33)
    assert st == A.ERR_INVALID_ARG and "32-bit" in msg
    st, msg = call(n=101)
    assert st == A.ERR_INVALID_ARG and "capacity" in msg
    for entries in (-1, 2**31):
        st, msg = call(entries=entries)
        assert st == A.ERR_INVALID_ARG and "entry_count" in msg, entries
    st, msg = call(keys=_keys(0, 1), nk=2, entries=10)
    assert st == A.ERR_INVALID_ARG and "entry_count" in msg and "2 keys" in msg
    for bucket in (0, -86400):
        st, msg = call(bucket=bucket)
        assert st == A.ERR_INVALID_ARG and "bucket" in msg, bucket
    st, msg = call(flags=2)
    assert st == A.ERR_INVALID_ARG and "flags" in msg
    for kw in ({}, {"keys": _keys(0, 2), "nk": 2, "entries": 0}):
        need = L.hdk_hip_key_multiplicity_workspace_bytes(100, kw.get("keys", _keys(1)), kw.get("nk", 1), kw.get("entries", 100))
        assert need > 0
        st, msg = call(ws=1 << 24, ws_bytes=need - 1, **kw)
        assert st == A.ERR_INVALID_ARG and "workspace" in msg and "needed" in msg
        st, msg = call(ws=(1 << 24) + 4, ws_bytes=need, **kw)
        assert st == A.ERR_INVALID_ARG and "aligned" in msg
        st, msg = call(ws=4096 + 1024, ws_bytes=need, **kw)
        assert st == A.ERR_INVALID_ARG and "overlap" in msg and "workspace" in msg
    st, msg = call(rec=(1 << 20) + 4)
    assert st == A.ERR_INVALID_ARG and "aligned" in msg
    st, msg = call(rec=4096 + 16)
    assert st == A.ERR_INVALID_ARG and "overlap" in msg and "result" in msg
    # valid calls, given a device that does not exist: with these made-up addresses a call must never get as far as a launch
    for kw in ({}, {"flags": A.KEYS_NULLS_MATCH, "entries": 101}, {"bucket": 86400, "entries": 1}, {"cols": None, "n": 0, "cap": 0},
               {"keys": _keys(0, 1, 2), "nk": 3, "entries": 0}, {"entries": 0}, {"entries": 2**31 - 1}):
        st, msg = call(device=-1, **kw)
        assert st == A.ERR_INVALID_ARG and msg == "device -1 out of range", (kw, msg)


def test_workspace_arithmetic():
    L = lib()
    for n in (0, 1, 4096, 4097, 100_000):
        for keys, nk, entries in ((_keys(1), 1, 1), (_keys(1), 1, 100_000), (_keys(2), 1, 0), (_keys(0, 1), 2, 0),
                                  (_keys(2, 0, 1), 3, 0)):
            want = M.workspace_bytes(n, [M.key(keys[i].col) for i in range(nk)], entries,
                                     L.hdk_hip_sort_columns_workspace_bytes(n, nk))
            assert L.hdk_hip_key_multiplicity_workspace_bytes(n, keys, nk, entries) == want, (n, nk, entries)
    # spelled out: a perfect table of 100 slots is 400 bytes of counters -> 512, plus one 16-byte partial per block and pass
    assert L.hdk_hip_key_multiplicity_workspace_bytes(10, _keys(0), 1, 100) == 512 + 2 * 2048 * 16
    # the counters are the one-to-one table's size; the row count does not enter
    assert L.hdk_hip_key_multiplicity_workspace_bytes(1, _keys(0), 1, 1 << 20) == \
        L.hdk_hip_key_multiplicity_workspace_bytes(10**8, _keys(0), 1, 1 << 20) == (4 << 20) + 65536
    # the sorted temporary holds every column up to the highest key column
    a = L.hdk_hip_key_multiplicity_workspace_bytes(4096, _keys(0), 1, 0)
    b = L.hdk_hip_key_multiplicity_workspace_bytes(4096, _keys(2), 1, 0)
    assert b - a == 2 * 4096 * 8
    # what the call would refuse has no size
    for keys, nk, entries in ((None, 1, 0), (_keys(0), 0, 0), (_keys(0), 4, 0), (_keys(0, 1), 2, 5), (_keys(0), 1, -1), (_keys(-1), 1, 0)):
        assert L.hdk_hip_key_multiplicity_workspace_bytes(100, keys, nk, entries) == 0


def test_the_structs_and_constants_mirror_the_header():
    L = lib()
    assert C.sizeof(A.MultiplicityKey) == L.hdk_hip_sizeof_multiplicity_key() == 40
    assert C.sizeof(A.KeyMultiplicityResult) == L.hdk_hip_sizeof_key_multiplicity_result() == 32
    assert A.KEYS_NULLS_MATCH == 1 and A.MAX_JOIN_KEYS == 3


# ---- a DeviceTable with its number compiles to the plan of a host table with the same values -----------------------------
class FakeBlock:
    def __init__(self, ptr):
        self.ptr, self.freed = ptr, 0

    def free(self):
        self.freed += 1
        self.ptr = 0


def both_storages(fill=True):
    """-> (storage whose inner table "dimr" is a DeviceTable over a fake block, storage with the same values on the host);
    both hold the host fact table "f".  fill: key_multiplicity of every SPECS key, from the evaluator."""
    data = inner_columns()
    rng = np.random.default_rng(5)
    n = 2000
    fact = {"fk": rng.integers(0, 800, n).astype(np.int64), "fd": (rng.integers(-12, 22, n) * DAY).astype(np.int64),
            "fa": rng.integers(0, 8, n).astype(np.int64), "fb": rng.integers(-3, 8, n).astype(np.int64),
            "fc": rng.integers(0, 2, n).astype(np.int64), "val": rng.integers(0, 100, n).astype(np.int64)}
    ftypes = {"fk": I8N, "fd": DATE_S, "fa": I8N, "fb": I8N, "fc": I8N, "val": I8}
    host, dev = S.ArrowStorage(), S.ArrowStorage()
    for st in (host, dev):
        st.import_numpy("f", fact, fragment_size=700, types=ftypes)
    ht = host.import_numpy("dimr", data, fragment_size=256, types=TYPES)
    cols = [S.Column(nm, TYPES[nm], [], list(ht.columns[nm].stats)) for nm in ORDER]
    dt = dev.add_table(S.DeviceTable("dimr", cols, list(ht.frag_rows), FakeBlock(1 << 30), 608, 256, joinable=True))
    if fill:
        for spec in SPECS.values():
            shape, got = evaluate(ht, data, spec)
            dt.key_multiplicity[shape.multiplicity_key] = got[:2]
    return dev, host


def _unit(spec, project=False, jtype="inner"):
    import dataclasses
    spec = dataclasses.replace(spec, type=jtype)
    if jtype in ("semi", "anti"):
        return QueryUnit("f", joins=[spec], targets=[Agg("sum", ColRef("val"), "s"), Agg("count", None, "c")])
    if project:
        return QueryUnit("f", joins=[spec], targets=[Proj(ColRef("val"), "val"), Proj(ColRef("v", "dimr"), "v")])
    return QueryUnit("f", joins=[spec], groupby=[ColRef("fa")],
                     targets=[KeyRef(0, "fa"), Agg("sum", BinOp("+", ColRef("val"), ColRef("v", "dimr")), "s")])


PLANS = {
    "one_to_one": (_unit(SPECS["unique"]), A.JOIN_ONE_TO_ONE),
    "one_to_many": (_unit(SPECS["many"]), A.JOIN_ONE_TO_MANY),
    "null_safe": (_unit(SPECS["many_null_safe"]), A.JOIN_ONE_TO_MANY),
    "date": (_unit(SPECS["date"]), A.JOIN_ONE_TO_MANY),
    "keyed_two": (_unit(SPECS["two"]), A.JOIN_KEYED_ONE_TO_MANY),
    "left_projection": (_unit(SPECS["many"], project=True, jtype="left"), A.JOIN_ONE_TO_MANY),
    "projection_one_to_one": (_unit(SPECS["unique"], project=True), A.JOIN_ONE_TO_ONE),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_a_device_inner_table_compiles_to_the_plan_of_the_host_table(name):
    dev, host = both_storages()
    unit, kind = PLANS[name]
    a, b = compile_query(dev, unit), compile_query(host, unit)
    assert bytes(a.plan) == bytes(b.plan)
    assert a.join_infos == b.join_infos and a.join_infos[0]["kind"] == kind
    assert a.entry_count == b.entry_count and a.buffer_bytes == b.buffer_bytes
    assert a.input_cols == b.input_cols and a.slot_widths == b.slot_widths and a.inner_tables == b.inner_tables
    if name == "left_projection":  # the entry count carries the fan-out
        one = compile_query(host, PLANS["projection_one_to_one"][0])
        assert a.join_infos[0]["max_matches"] > 1 and a.entry_count == one.entry_count * a.join_infos[0]["max_matches"]


@pytest.mark.parametrize("jtype", ["semi", "anti"])
@pytest.mark.parametrize("spec", ["many", "two"])
def test_semi_and_anti_joins_need_no_number(jtype, spec):
    dev, host = both_storages(fill=False)
    assert dev.get("dimr").key_multiplicity == {}
    unit = _unit(SPECS[spec], jtype=jtype)
    a, b = compile_query(dev, unit), compile_query(host, unit)
    assert bytes(a.plan) == bytes(b.plan) and a.join_infos == b.join_infos and a.buffer_bytes == b.buffer_bytes
    assert a.join_infos[0]["kind"] in (A.JOIN_ONE_TO_ONE, A.JOIN_KEYED_ONE_TO_ONE)


@pytest.mark.parametrize("name", sorted(PLANS))
def test_without_the_number_compile_query_keeps_its_refusal(name):
    dev, _ = both_storages(fill=False)
    with pytest.raises(QueryMustRunOnCpu, match="^a registered result can only be scanned as the outer table$"):
        compile_query(dev, PLANS[name][0])


def test_a_number_for_another_key_does_not_serve():
    dev, _ = both_storages(fill=False)
    dev.get("dimr").key_multiplicity[multiplicity_key(["k"], True, 1)] = (9, 9)  # (the null-safe key: not the plain one)
    with pytest.raises(QueryMustRunOnCpu, match="outer table"):
        compile_query(dev, PLANS["one_to_many"][0])
    dev.get("dimr").key_multiplicity[multiplicity_key(["k"], False, 1)] = (0, 0)  # no row filed reads as 1, like the host's
    assert compile_query(dev, PLANS["one_to_many"][0]).join_infos[0]["kind"] == A.JOIN_ONE_TO_ONE


def test_an_empty_inner_table_keeps_its_refusal():
    dev = S.ArrowStorage()
    dev.import_numpy("f", {"fk": np.arange(10, dtype=np.int64)})
    col = S.Column("k", I8N, [], [S.ChunkStats(None, None, False)])
    dev.add_table(S.DeviceTable("dimr", [col], [0], FakeBlock(1 << 30), 32, 32, joinable=True))
    q = QueryUnit("f", joins=[JoinSpec("dimr", ColRef("fk"), "k")], targets=[Agg("count", None, "c")])
    with pytest.raises(QueryMustRunOnCpu, match="empty join inner table"):
        compile_query(dev, q)
    with pytest.raises(QueryMustRunOnCpu, match="empty join inner table"):
        Executor(dev, 0, mgr=object()).compile(q)  # (nothing is measured: the manager is never asked)


# ---- the executor's host side ---------------------------------------------------------------------------------------------
class FakeBuffer:
    def __init__(self):
        self.freed = 0

    def free(self):
        self.freed += 1


def test_compile_measures_nothing_that_is_there_or_not_needed():
    dev, host = both_storages()
    ex = Executor(dev, 0, mgr=object())  # (a measurement would ask the manager for memory and fail)
    for name, (unit, _) in PLANS.items():
        assert bytes(ex.compile(unit).plan) == bytes(compile_query(host, unit).plan), name
    bare, _ = both_storages(fill=False)
    ex = Executor(bare, 0, mgr=object())
    ex.compile(_unit(SPECS["many"], jtype="semi"))
    with pytest.raises(AttributeError):  # the plain join asks the device: this stand-in has none
        ex.compile(PLANS["one_to_many"][0])
    assert bare.get("dimr").key_multiplicity == {}


def test_drop_registered_empties_both_join_caches_of_that_name():
    dev, _ = both_storages()
    ex = Executor(dev, 0, mgr=object())
    mine = [FakeBuffer() for _ in range(4)]
    other = [FakeBuffer() for _ in range(2)]
    ex._join_cache[("dimr", ("k",), A.JOIN_ONE_TO_MANY, 0, 0)] = mine[0]
    ex._join_cache[("dimr", ("a", "b"), A.JOIN_KEYED_ONE_TO_MANY, 0, 0)] = mine[1]
    ex._join_cache[("dim", ("dimr",), A.JOIN_ONE_TO_ONE, 0, 0)] = other[0]  # (another table; the name only as a column)
    ex._fused_cache[("dimr", "u", ("v",), 0, 0)] = mine[2]
    ex._fused_cache[("dimr", "u", ("v", "k"), 0, 0)] = mine[3]
    ex._fused_cache[("dim", "dk", ("dval",), 0, 0)] = other[1]
    block = dev.get("dimr").block
    ex.drop_registered("dimr")
    assert "dimr" not in dev.tables and block.freed == 1
    assert [b.freed for b in mine] == [1, 1, 1, 1] and [b.freed for b in other] == [0, 0]
    assert list(ex._join_cache) == [("dim", ("dimr",), A.JOIN_ONE_TO_ONE, 0, 0)]
    assert list(ex._fused_cache) == [("dim", "dk", ("dval",), 0, 0)]


def test_compile_refuses_a_join_against_a_unit():
    dev, _ = both_storages()
    sub = QueryUnit("dimr", groupby=[ColRef("k")], targets=[KeyRef(0, "k"), Agg("sum", ColRef("v"), "s")])
    q = QueryUnit("f", joins=[JoinSpec(sub, ColRef("fk"), "k")], targets=[Agg("sum", ColRef("s"), "t")])
    with pytest.raises(ValueError, match="execute"):
        Executor(dev, 0, mgr=object()).compile(q)


def test_a_table_registered_without_joinable_keeps_its_refusal():
    """what was registered as every result was before stays the outer table only: with the number there, and for a semi join"""
    dev, _ = both_storages()
    t = dev.get("dimr")
    assert t.joinable and S.DeviceTable("x", [], [0], FakeBlock(1), 32, 32).joinable is False
    t.joinable = False
    for unit in (PLANS["one_to_one"][0], _unit(SPECS["many"], jtype="semi")):
        with pytest.raises(QueryMustRunOnCpu, match="^a registered result can only be scanned as the outer table$"):
            compile_query(dev, unit)
        with pytest.raises(QueryMustRunOnCpu, match="outer table"):
            Executor(dev, 0, mgr=object()).compile(unit)  # (nothing is measured: the manager is never asked)
