"""The numpy statement of hdk_hip_key_multiplicity's contract (include/hdk_hip.h): both routes, the NULL rules,
rows_out_of_range, occupied.  A key is (col, nullable, null_bits, min_val, max_val, translated_null); the answer is
(max_matches, occupied, rows_filed, rows_out_of_range)."""
import numpy as np

NULL_I64 = np.int64(-(2**63))
TILE = 4096
GRID_MAX = 2048


def key(col, nullable=True, null_bits=int(NULL_I64), min_val=0, max_val=0, translated_null=None):
    return (col, bool(nullable), int(null_bits), int(min_val), int(max_val), int(max_val) + 1 if translated_null is None else
            int(translated_null))


def perfect(cols, n, k, entry_count, bucket=1, nulls_match=False):
    """One key over a perfect table of `entry_count` slots: fill_hash_join_buff_impl restated.  A NULL word is dropped, or
    filed under translated_null; a non-NULL word outside [min_val, max_val] or a slot outside the table is out of range."""
    col, nullable, null_bits, mn, mx, tr = k
    filed, outside = {}, 0
    for w in (int(x) for x in np.asarray(cols[col][:n], dtype=np.int64)):
        is_null = nullable and w == null_bits
        if is_null and not nulls_match:
            continue
        elem = tr if is_null else w
        if not is_null and not mn <= elem <= mx:
            outside += 1
            continue
        slot = (elem - mn) // bucket if elem >= mn else -1  # (C++: an unsigned compare sends a negative difference outside)
        if not 0 <= slot < entry_count:
            outside += 1
            continue
        filed[slot] = filed.get(slot, 0) + 1
    return (max(filed.values(), default=0), len(filed), sum(filed.values()), outside)


def sorted_route(cols, n, keys):
    """1..3 components: a row with a NULL in any component is skipped; rows match when every component word is equal."""
    filed = {}
    arrs = [np.asarray(cols[k[0]][:n], dtype=np.int64) for k in keys]
    for r in range(n):
        t = tuple(int(a[r]) for a in arrs)
        if any(k[1] and w == k[2] for k, w in zip(keys, t)):
            continue
        filed[t] = filed.get(t, 0) + 1
    return (max(filed.values(), default=0), len(filed), sum(filed.values()), 0)


def expect(cols, n, keys, entry_count=0, bucket=1, nulls_match=False):
    if entry_count > 0:
        assert len(keys) == 1
        return perfect(cols, n, keys[0], entry_count, bucket, nulls_match)
    return sorted_route(cols, n, keys)


def _align256(x):
    return (x + 255) // 256 * 256


def workspace_bytes(n, keys, entry_count, sort_workspace_bytes):
    """`sort_workspace_bytes`: hdk_hip_sort_columns_workspace_bytes(n, len(keys)), the library's own sort's need"""
    if n == 0:
        return 0
    if entry_count > 0:
        return _align256(entry_count * 4) + 2 * GRID_MAX * 16
    sort_cols = max(k[0] for k in keys) + 1
    return (_align256(sort_cols * ((n + 31) // 32 * 32) * 8) + _align256(sort_workspace_bytes)
            + _align256(-(-n // TILE) * 32))
