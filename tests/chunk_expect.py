"""hdk_hip_chunk_columns stated in numpy: the copy with the NULL rewrite, and the per-fragment statistics with the NaN rule
(include/hdk_hip.h has the contract).  Shared by the CPU and the GPU tests of the call."""
import numpy as np

NULL_I64 = np.int64(-2**63)
NULL_I32 = np.int64(-2**31)  # a 4-byte slot's sentinel sign-extended
NULL_DOUBLE_BITS = np.array([np.finfo(np.float64).tiny], dtype=np.float64).view(np.int64)[0]
NULL_FLOAT_WIDE_BITS = np.array([np.float64(np.finfo(np.float32).tiny)], dtype=np.float64).view(np.int64)[0]  # FLT_MIN widened
POS_INF_BITS = np.array([np.inf], dtype=np.float64).view(np.int64)[0]
NEG_INF_BITS = np.array([-np.inf], dtype=np.float64).view(np.int64)[0]


def num_fragments(num_rows, fragment_rows):
    return max(1, -(-num_rows // fragment_rows))


def tiles(num_rows, fragment_rows, tile=4096):
    """tiles are cut at fragment boundaries: every fragment but the last has ceil(fragment_rows / tile), the last its own"""
    if num_rows == 0:
        return 0
    nf = num_fragments(num_rows, fragment_rows)
    return (nf - 1) * -(-fragment_rows // tile) + -(-(num_rows - (nf - 1) * fragment_rows) // tile)


def workspace_bytes(num_rows, fragment_rows, num_cols):
    return (num_cols * tiles(num_rows, fragment_rows) * 32 + 255) & ~255


def copy(cols, num_rows, sel):
    """`cols`: the input columns as int64 words; `sel`: (col, is_fp, nullable, null_bits, out_null_bits) per output column
    -> the output columns, rows [0, num_rows)"""
    out = []
    for col, _is_fp, nullable, null_bits, out_null in sel:
        w = np.asarray(cols[col], dtype=np.int64)[:num_rows].copy()
        if nullable:
            w[w == np.int64(null_bits)] = np.int64(out_null)
        out.append(w)
    return out


def stats(out, sel, num_rows, fragment_rows):
    """-> stats[j][f] = (min_bits, max_bits, null_count, value_count) over the OUTPUT words; min_bits / max_bits are None when
    no value took part (no non-NULL word; for an fp column also: NaNs only).  An fp min / max is the bit pattern of A value
    that compares equal to the extreme (-0.0 and +0.0 are one value): compare with same_stats()."""
    res = []
    for w, (_col, is_fp, nullable, _null_bits, out_null) in zip(out, sel):
        per = []
        for f in range(num_fragments(num_rows, fragment_rows)):
            x = w[f * fragment_rows:min((f + 1) * fragment_rows, num_rows)]
            null = (x == np.int64(out_null)) if nullable else np.zeros(len(x), dtype=bool)
            v = x[~null]
            if is_fp:
                d = v.view(np.float64)
                d = d[~np.isnan(d)]
                mn, mx = (None, None) if d.size == 0 else (int(np.array([d.min()]).view(np.int64)[0]),
                                                            int(np.array([d.max()]).view(np.int64)[0]))
            else:
                mn, mx = (None, None) if v.size == 0 else (int(v.min()), int(v.max()))
            per.append((mn, mx, int(null.sum()), int(v.size)))
        res.append(per)
    return res


def same_stats(got, want, is_fp):
    """a device record (min_bits, max_bits, null_count, value_count) against stats()'s tuple"""
    if (int(got[2]), int(got[3])) != (want[2], want[3]):
        return False
    if want[3] == 0:
        return True  # (min / max are meaningful only with a value)
    if want[0] is None:  # NaNs only
        return is_fp and int(got[0]) == int(POS_INF_BITS) and int(got[1]) == int(NEG_INF_BITS)
    if is_fp:
        g = np.array([got[0], got[1]], dtype=np.int64).view(np.float64)
        e = np.array([want[0], want[1]], dtype=np.int64).view(np.float64)
        return bool(g[0] == e[0] and g[1] == e[1])
    return (int(got[0]), int(got[1])) == (want[0], want[1])
