"""Minimal plan IR for the hot path: types, expressions and the query unit the executor consumes.

It is the flattened stand-in for HDK's `RelAlgExecutionUnit` (reference
omniscidb/QueryEngine/RelAlgExecutionUnit.h): input columns, simple_quals/quals, join quals,
groupby_exprs, target_exprs.  The full `hdk::ir` DAG (omniscidb/IR/) stays out of scope; a real
integration pattern-matches its work unit into this shape.
"""
from dataclasses import dataclass, field
from typing import Sequence, List, Optional, Union

from . import _abi as A


class QueryMustRunOnCpu(Exception):
    """Plan shape outside the fixed kernel library (reference QueryEngine/ErrorHandling.h;
    caught by RelAlgExecutor::executeRelAlgQuery, RelAlgExecutor.cpp:183-192)."""


# ---------------------------------------------------------------------------------------------
# types
# ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Type:
    """Subset of hdk::ir::Type (omniscidb/IR/Type.h): fixed-width, in-band-null columns."""
    kind: str  # 'int' | 'fp' | 'decimal' | 'timestamp' | 'date' | 'dict' | 'bool'
    size: int  # bytes
    nullable: bool = True
    scale: int = 0  # decimal scale
    unit: str = "s"  # timestamp / date unit; a DATE in days (unit 'd', 2 or 4 bytes: Arrow date32, hdk::ir::DateType with
    #                  TimeUnit::kDay) is read as epoch seconds by fixed_width_small_date_decode (QE/ColumnIR.cpp:46-49)

    @property
    def is_fp(self):
        return self.kind == "fp"

    @property
    def is_integer_like(self):
        return self.kind in ("int", "decimal", "timestamp", "date", "dict", "bool")

    @property
    def is_date_in_days(self):
        return self.kind == "date" and self.unit == "d"

    def logical(self) -> "Type":
        """The type expressions see (hdk::ir::Type::canonicalize): a DATE in days is an 8-byte DATE in seconds once
        decoded, with NULL_BIGINT for the column's narrow NULL (FixedWidthSmallDate, QE/Codec.cpp:86-102)."""
        return Type("date", 8, self.nullable, 0, "s") if self.is_date_in_days else self

    def with_nullable(self, n):
        return Type(self.kind, self.size, n, self.scale, self.unit)

    def null_value(self) -> int:
        """In-band null sentinel (omniscidb/Shared/InlineNullValues.h:33-39): the int value, or the
        bit pattern for fp."""
        if self.is_fp:
            return A.NULL_DOUBLE_BITS if self.size == 8 else A.NULL_FLOAT_BITS
        return -(1 << (8 * self.size - 1))

    def null_as_int64_or_double_bits(self) -> int:
        """Null sentinel after the column has been widened by the decoder: ints sign-extend, floats
        are widened to double (FLT_MIN as a double)."""
        if self.is_fp:
            if self.size == 8:
                return A.NULL_DOUBLE_BITS
            import struct
            f = struct.unpack("<f", struct.pack("<I", A.NULL_FLOAT_BITS))[0]
            return struct.unpack("<q", struct.pack("<d", float(f)))[0]
        return self.null_value()


def int_type(size, nullable=True):
    return Type("int", size, nullable)


INT64 = int_type(8)
INT32 = int_type(4)
INT16 = int_type(2)
INT8 = int_type(1)
DATE32 = Type("date", 4, True, 0, "d")  # Arrow date32: days, 4 bytes (ArrowStorageUtils.cpp:899-914)
DATE16 = Type("date", 2, True, 0, "d")
DATE64 = Type("date", 8, True, 0, "s")  # a DATE held in seconds: plain integer decode, still bucketized by day
FP64 = Type("fp", 8)
FP32 = Type("fp", 4)


# ---------------------------------------------------------------------------------------------
# expressions
# ---------------------------------------------------------------------------------------------
class Expr:
    def __add__(self, o):
        return BinOp("+", self, _lit(o))

    def __sub__(self, o):
        return BinOp("-", self, _lit(o))

    def __mul__(self, o):
        return BinOp("*", self, _lit(o))

    def __truediv__(self, o):
        return BinOp("/", self, _lit(o))

    def __mod__(self, o):
        return BinOp("%", self, _lit(o))


def _lit(v):
    return v if isinstance(v, Expr) else Lit(v)


@dataclass(frozen=True)
class ColRef(Expr):
    """Column of the outer table (table=None / scan table name) or of a joined inner table."""
    name: str
    table: Optional[str] = None


@dataclass(frozen=True)
class Lit(Expr):
    value: Union[int, float]


@dataclass(frozen=True)
class TargetRef(Expr):
    """A target of the same step, by 0-based index or output name: what a HAVING comparison reads (the reference's
    filter step over the previous step's result names that result's columns).  Valid only inside QueryUnit.having:
    compile_query raises a ValueError for one in quals, groupby, targets or join keys.  Inside QueryUnit.select it names a
    column of the result that the projection reads: a target or a window column."""
    target: Union[int, str]


@dataclass(frozen=True)
class BinOp(Expr):
    op: str  # + - * / %
    lhs: Expr
    rhs: Expr


@dataclass(frozen=True)
class ExtractYear(Expr):
    """extract(year from <timestamp>) -- omniscidb/Utils/ExtractFromTime.cpp:260-272."""
    arg: Expr


@dataclass(frozen=True)
class Cast(Expr):
    """cast(<expr> as <to>): decimal->int (rounded scale down), int->fp, fp->int."""
    arg: Expr
    to: Type


@dataclass(frozen=True)
class Cmp:
    """Filter conjunct lhs <op> rhs with rhs a literal or a column."""
    lhs: Expr
    op: str  # = <> < > <= >=
    rhs: Expr


@dataclass(frozen=True)
class And:
    """lhs AND rhs over filter conditions, three-valued (logical_and, QE/RuntimeFunctions.cpp:361-372)."""
    lhs: "Cond"
    rhs: "Cond"


@dataclass(frozen=True)
class Or:
    """lhs OR rhs, three-valued (logical_or, QE/RuntimeFunctions.cpp:374-384)."""
    lhs: "Cond"
    rhs: "Cond"


@dataclass(frozen=True)
class Not:
    """NOT arg, three-valued (logical_not, QE/RuntimeFunctions.cpp:355-358)."""
    arg: "Cond"


@dataclass(frozen=True)
class IsNull:
    """arg IS NULL: a condition that is never NULL itself.  Valid inside QueryUnit.select (DeviceColumns.project)."""
    arg: Expr


Cond = Union[Cmp, And, Or, Not, IsNull]


@dataclass(frozen=True)
class Case(Expr):
    """CASE WHEN cond THEN expr [WHEN ...] [ELSE else_] END (hdk::ir::CaseExpr): the first `whens` pair whose condition is
    TRUE gives the value; a FALSE or NULL condition moves on; without `else_` (or with Lit(None) for it) the rest is NULL.
    A branch that is Lit(None) is a NULL of the other branches' type.  Valid inside QueryUnit.select."""
    whens: Sequence  # of (Cond, Expr)
    else_: Optional[Expr] = None


@dataclass(frozen=True)
class Agg:
    """Aggregate target: kind in count/sum/min/max/avg/single_value; arg None = COUNT(*).  kind count_distinct
    (COUNT(DISTINCT arg)) is valid in a group-by unit run with Executor.execute(result="columns"), which runs it as
    GROUP BY keys, arg followed by a regroup of the dense columns by the keys (plan.split_count_distinct)."""
    kind: str
    arg: Optional[Expr] = None
    name: Optional[str] = None


@dataclass(frozen=True)
class KeyRef:
    """Non-aggregate target projecting group-by key #idx."""
    idx: int
    name: Optional[str] = None


@dataclass(frozen=True)
class Proj:
    """Projected expression of a filter/project step (no GROUP BY, no aggregates)."""
    expr: Expr
    name: Optional[str] = None


@dataclass(frozen=True)
class JoinSpec:
    """Equi-join of the outer table with `inner_table` on outer_key == inner_col.  Both sides may be
    lists of equal length (composite key -> keyed/"baseline" hash table, BaselineJoinHashTable); the
    table kind (one-to-one / one-to-many, perfect / keyed) is chosen from the inner table's data the
    way PerfectJoinHashTable::reify / HashJoin::getInstance do (QE/JoinHashTable/HashJoin.cpp:258-330).
    `inner_table` names a table of the storage -- a result registered with joinable=True (Executor.register_columns) included, whose key
    multiplicity Executor.compile measures on the device -- or is itself a QueryUnit, a join against a subquery, which
    Executor.execute runs first and joins where it lies (Executor.compile refuses such a unit)."""
    inner_table: Union[str, "QueryUnit"]
    outer_key: Union[Expr, Sequence[Expr]]
    inner_col: Union[str, Sequence[str]]
    type: str = "inner"  # inner | left | semi | anti  (JoinType, Shared/sqldefs.h:33)
    # outer_key IS NOT DISTINCT FROM inner_col (hdk::ir::OpType::kBwEq): NULL keys match NULL keys -- the build files
    # them under a translated value and the probe is hash_join_idx_bitwise (PerfectJoinHashTable.cpp:798-816)
    null_safe: bool = False

    @property
    def outer_keys(self) -> list:
        return list(self.outer_key) if isinstance(self.outer_key, (list, tuple)) else [self.outer_key]

    @property
    def inner_cols(self) -> list:
        return list(self.inner_col) if isinstance(self.inner_col, (list, tuple)) else [self.inner_col]


@dataclass(frozen=True)
class OrderEntry:
    """One ORDER BY entry (hdk::ir::OrderEntry, omniscidb/IR/Node.h: tle_no, is_desc, nulls_first): `target` is the
    target's 0-based index or its output name."""
    target: Union[int, str]
    desc: bool = False
    nulls_first: bool = False


WINDOW_KINDS = ("row_number", "rank", "dense_rank", "percent_rank", "cume_dist", "ntile", "lag", "lead", "first_value",
                "last_value", "avg", "min", "max", "sum", "count")  # hdk::ir::WindowFunctionKind, IR/OpTypeEnums.h:95-112
WINDOW_FRAMES = ("rows", "range", "partition")


@dataclass(frozen=True)
class Window:
    """One window function over the unit's result columns (hdk::ir::WindowFunction): kind in WINDOW_KINDS OVER (PARTITION
    BY partition_by ORDER BY order_by).  `arg` and the partition keys name OUTPUT columns: a TargetRef, a target index or
    an output name (arg None: COUNT(*), and the ranking kinds take none).  `frame`: every frame starts at the partition's
    first row and ends at the row itself ("rows"), at its last peer ("range") or at the partition's last row
    ("partition"); None takes the reference's default -- "partition" without order entries, else "range" for count / sum /
    avg and "rows" for min / max / last_value.  `param`: NTILE's n, LAG / LEAD's k (default 1), a constant."""
    kind: str
    arg: Optional[Union[Expr, int, str]] = None
    partition_by: Sequence = ()
    order_by: Sequence["OrderEntry"] = ()
    frame: Optional[str] = None
    param: Optional[Union[int, Expr]] = None
    name: Optional[str] = None


@dataclass(frozen=True, eq=False)
class ResultJoin:
    """A join of the unit's result columns with another result that already sits on the device (the reference joins a
    registered ResultSet like any table, QE/ColumnFetcher.cpp:111): `right` is an executor.DeviceColumns, which is not
    consumed; `left_on` / `right_on` name the key columns of the unit's result / of `right` by index or output name
    (right_on None: the same as left_on); `type` is inner, left, semi or anti; `null_safe` makes a NULL key match a NULL
    key (IS NOT DISTINCT FROM); `right_cols` picks the columns of `right` that follow the unit's own, as columns or
    (column, new name) pairs (None: every column that is not a key; none for semi / anti)."""
    right: object
    left_on: Sequence
    right_on: Optional[Sequence] = None
    type: str = "inner"
    null_safe: bool = False
    right_cols: Optional[Sequence] = None


@dataclass(frozen=True, eq=False)
class ResultSetOp:
    """A set operation of the unit's result columns (the LEFT operand) with another result that already sits on the device
    (the reference's LogicalUnion over two previous steps' results, widened to SQL's other set operations): `right` is an
    executor.DeviceColumns, which is not consumed; `op` is union, intersect or except; `all` keeps duplicates (UNION ALL,
    INTERSECT ALL, EXCEPT ALL).  Columns pair by position and whole rows are compared (plan.resolve_setop_columns)."""
    right: object
    op: str
    all: bool = False


@dataclass
class QueryUnit:
    """What one execution step needs (cf. RelAlgExecutionUnit).  `table` names a table of the storage, or is itself a
    QueryUnit -- a FROM-subquery, which Executor.execute runs first and scans where it lies, in device memory; a
    JoinSpec's inner_table may be one too (Executor.compile refuses either unit: its plan needs the inner result's
    statistics).  A registered result is the outer table, and one registered as joinable also the inner table of a join."""
    table: Union[str, "QueryUnit"]
    quals: List[Cond] = field(default_factory=list)  # conjunction of conditions (each a Cmp or an And / Or / Not tree)
    joins: List[JoinSpec] = field(default_factory=list)
    groupby: List[Expr] = field(default_factory=list)
    targets: List[Union[Agg, KeyRef, Proj]] = field(default_factory=list)
    scan_limit: Optional[int] = None  # projection: max output rows (RelAlgExecutionUnit::scan_limit)
    # hints (ExecutionOptions / Config.exec.group_by)
    output_columnar: bool = False
    bigint_count: bool = False  # Config.exec.group_by.bigint_count (omniscidb/Shared/Config.h:44)
    baseline_entry_count: Optional[int] = None  # max_groups_buffer_entry_count override
    force_baseline: bool = False
    # SortInfo (RelAlgExecutionUnit::sort_info): applied to the dense result columns on the device (result="columns")
    order_by: List[OrderEntry] = field(default_factory=list)
    limit: Optional[int] = None
    offset: int = 0
    # HAVING: a conjunction of Cmp / And / Or / Not trees whose leaves are Cmp(TargetRef, op, Lit) or
    # Cmp(TargetRef, op, TargetRef) (a literal on the left is swapped, the operator mirrored); applied to the dense result
    # columns on the device before order_by / limit / offset (result="columns")
    having: List[Cond] = field(default_factory=list)
    # window functions over the result columns, applied on the device after HAVING and before order_by / limit / offset
    # (result="columns"): each adds a column after the targets, in this order; order_by may name one
    windows: List[Window] = field(default_factory=list)
    # the final projection: Proj(expr, name) items over the result columns (targets and window columns, by TargetRef), applied
    # on the device after HAVING and the windows and before order_by / limit / offset (result="columns"), whose entries then
    # name the PROJECTED columns.  The result holds these columns only.  Empty: every column as it is
    select: List["Proj"] = field(default_factory=list)
    # set operations of the result columns with other device results (the unit's result is the left operand), applied on
    # the device in order after the select list and before order_by / limit / offset, which then apply to the COMBINED
    # rows, as a compound query's ORDER BY does (result="columns").  It stands before result_joins, which
    # stays the last field
    result_setops: List[ResultSetOp] = field(default_factory=list)
    # joins of the result columns with other device results, applied on the device FIRST, in order (result="columns"):
    # having, windows, select and order_by may then name a joined column
    result_joins: List[ResultJoin] = field(default_factory=list)
