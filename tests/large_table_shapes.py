"""The shapes of the large-table tests (a plain module: no tests in it), and the address arithmetic they stand on.

Every gather kernel addresses a row as an unsigned 32-bit count of PIECES from its table's base (csrc/sls_dev.h
`E::row_piece`): 16-byte pieces for fp32 / fp16 / bf16 / fp8 rows, 4-byte pieces for int8 rowwise rows, 2-byte pieces for
int4 rowwise rows.  Only the rowwise types can reach a piece offset with bit 31 set (drs_create keeps rows * D < 2^33, so the
others stay below 2^31; convert_tables keeps the rowwise ones below 2^32).  tests/test_large_tables.py (GPU) runs tables
whose LAST rows sit there; tests/test_large_tables_cpu.py holds the constants below to their edges, so that an edit cannot
move a case off its edge unnoticed.

The arithmetic is restated in plain Python from DESIGN.md 2 and csrc/drs_internal.h (table_row_stride, row_lines,
i8_row_offset, i8_table_bytes, table_layout) and csrc/engine_options.hip (convert_tables' two refusals and its memory rule).
"""
import numpy as np

from oracle import oracle as orc

FP32, FP16, BF16, FP8, I8, I4 = 0, 1, 2, 4, 8, 9       # "table_dtype" values (deeprecsys_amd._native.TABLE_*)

# ---- the shapes -------------------------------------------------------------------------------------------------------
PIECES = 10                                   # pieces per row of both rowwise types at D 32 and D 30
D_MAIN, D_ANY = 32, 30                        # every 16-byte form | sls_any_kernel (30 % 4 != 0), the same strides
R_STAR = -(-(1 << 31) // PIECES)              # 214 748 365: the first row whose plain piece offset has bit 31 set
R_BIG = R_STAR + 4096                         # 214 752 461 rows: the last 4096 rows lie beyond R_STAR
R_STAR_LINES = 3 << 26                        # 201 326 592: the same edge in either line-packed layout
ROWS_A = (R_BIG, 1000)                        # table 1 sits BEHIND the big one: its tab_off exceeds 2^32 units
B, L_MAX = 64, 20
FILL = (-0.05, 0.05, 23)                      # fill_table_uniform(t, lo, hi, seed) of every table

D_LIMIT = 4                                   # 4 pieces per row for int8 (S 16) and for int4 (S 8)
ROWS_LIMIT = (1 << 30) - 1                    # accepted: the last row starts at piece 2^32 - 8
ROWS_REFUSED = 1 << 30                        # refused by both rules: 2^30 * 4 pieces = 2^32


# ---- the layouts, restated ----------------------------------------------------------------------------------------------
def row_stride(dtype, D):
    """bytes between the rows of a table (table_row_stride)"""
    if dtype == I4:
        return (D // 2 + 3) // 4 * 4 + 4      # code bytes padded to 4, fp16 scale and bias
    if dtype == I8:
        return (D + 7) // 8 * 8 + 8           # codes padded to 8, fp32 scale and bias
    return D * {FP32: 4, FP16: 2, BF16: 2, FP8: 1}[dtype]


def piece_bytes(dtype):
    return {I8: 4, I4: 2}.get(dtype, 16)


def pieces_per_row(dtype, D):
    """the row stride the kernels multiply by: int8 padded(D) / 4 + 2, int4 padded(D / 2) / 2 + 2, else D / 4 elements' worth"""
    if dtype == I8:
        return (D + 7) // 8 * 8 // 4 + 2
    if dtype == I4:
        return (D // 2 + 3) // 4 * 4 // 2 + 2
    return D // 4


def lines(dtype, D, packed):
    """(n, pad): rows per 128-byte line and the pieces that close a line -- (0, 0) for the plain layout (option off, S >= 128,
    or S divides 128)"""
    S = row_stride(dtype, D)
    if not packed or dtype not in (I8, I4) or S >= 128 or 128 % S == 0:
        return 0, 0
    n = 128 // S
    return n, 128 // piece_bytes(dtype) - n * (S // piece_bytes(dtype))


def row_piece(dtype, D, r, packed=False):
    """where row r starts in its table, in pieces -- as an unbounded integer (the kernels hold it in 32 bits)"""
    n, pad = lines(dtype, D, packed)
    return r * pieces_per_row(dtype, D) + ((r // n) * pad if n else 0)


def row_byte(dtype, D, r, packed=False):
    """byte offset of row r in its table (i8_row_offset for the rowwise types)"""
    S = row_stride(dtype, D)
    n, _ = lines(dtype, D, packed)
    return r // n * 128 + r % n * S if n else r * S


def row_at_piece(dtype, D, p, packed=False):
    """the row whose bytes hold piece p (a line's closing pieces count to its last row)"""
    n, _ = lines(dtype, D, packed)
    pr = pieces_per_row(dtype, D)
    if not n:
        return p // pr
    per_line = 128 // piece_bytes(dtype)
    return p // per_line * n + min(p % per_line // pr, n - 1)


def table_bytes(dtype, rows, D, packed=False):
    """bytes of one rowwise table before the arena's rounding (i8_table_bytes)"""
    n, _ = lines(dtype, D, packed)
    return -(-rows // n) * 128 if n else rows * row_stride(dtype, D)


def too_large(dtype, rows, D, packed=False):
    """convert_tables' refusals: an int8 table of 2^32 4-byte pieces or more, an int4 table of 2^32 2-byte pieces or more"""
    return dtype in (I8, I4) and table_bytes(dtype, rows, D, packed) // piece_bytes(dtype) >= 1 << 32


def create_accepts(rows, D):
    """drs_create: rows * D < 2^33 per table; row numbers are int32 on the device"""
    return rows * D < 1 << 33 and rows < 1 << 31


def table_offsets(dtype, rows, D, packed=False):
    """(offset of every table, arena bytes): the offsets count bytes for the rowwise types and fp8 (each table rounded up to
    256), elements otherwise (each table rounded up to 64) -- table_layout"""
    off, o = [], 0
    for r in rows:
        off.append(o)
        if dtype in (I8, I4, FP8):
            o += -(-(table_bytes(dtype, r, D, packed) if dtype != FP8 else r * D) // 256) * 256
        else:
            o += -(-r * D // 64) * 64
    return off, o * (1 if dtype in (I8, I4, FP8) else 4 if dtype == FP32 else 2)


def arena_bytes(dtype, rows, D, packed=False):
    return table_offsets(dtype, rows, D, packed)[1]


SLACK = 2 << 30      # what an engine of these tests holds besides its arena (batches, slots, weights: megabytes), rounded up


def free_needed(walk, rows, D):
    """Free device memory BEFORE the engine exists that lets every conversion of `walk` -- [(dtype, packed), ...], the first
    entry the arena drs_create allocates -- pass convert_tables' rule `new arena <= free / 4`, where `free` is read while the
    old arena is still held: the largest old + 4 * new over the walk's steps, plus SLACK."""
    need = arena_bytes(walk[0][0], rows, D, walk[0][1])
    for (a, pa), (b, pb) in zip(walk, walk[1:]):
        need = max(need, arena_bytes(a, rows, D, pa) + 4 * arena_bytes(b, rows, D, pb))
    return need + SLACK


# the arena states of Case A's walk, in order (tests/test_large_tables.py walks exactly these, in two tests; a fill changes no
# arena): steps 1 - 4, and steps 5 - 8 from step 4's state built again
WALK_A1 = ((FP32, False), (I8, False), (I8, True), (I8, False), (I4, False), (I4, True))
WALK_A2 = ((FP32, False), (I4, True), (FP16, False), (FP32, False), (BF16, False), (FP32, False), (FP8, False))


# ---- the rows the GPU cases pick ----------------------------------------------------------------------------------------
def half_cross(D):
    """the first row of an fp16 / bf16 table whose byte offset needs bit 32"""
    return -(-(1 << 31) // D)


def fp8_cross(D):
    """... of an fp8 table"""
    return -(-(1 << 32) // D)


def edges_a(D):
    """rows of table 0 that Case A's bags straddle, besides the table's two ends"""
    return (R_STAR, R_STAR_LINES, half_cross(D), fp8_cross(D))


def _straddle(edge, L):
    return np.arange(edge - L // 2, edge - L // 2 + L, dtype=np.int64)


def special_bags(rows, L, edges):
    """bags of exactly L rows: the table's last L rows, its first L, and L rows straddling every edge"""
    out = [np.arange(rows - L, rows, dtype=np.int64), np.arange(L, dtype=np.int64)]
    out += [_straddle(e, L) for e in edges]
    return out


def batches(rows, edges, high_from, seed):
    """The three staged batches of a case over tables of `rows` rows each, bags of table 0 as the issue lists them: batch 0
    one row per bag, batch 1 fixed L_MAX, batch 2 ragged 0 ... L_MAX with empty bags.  -> [(idx per table, lens per table)].
    The random rows of table 0 are drawn half from [high_from, rows) -- beyond the edge -- and half from the whole table."""
    rng = np.random.RandomState(seed)
    T = len(rows)

    def rand0(n):
        hi = rng.randint(high_from, rows[0], size=n).astype(np.int64)
        lo = (rng.randint(0, 1 << 30, size=n).astype(np.int64) * rows[0]) >> 30
        return np.where(rng.randint(0, 2, size=n) == 1, hi, lo)

    out = []
    for kind in ("one", "fixed", "ragged"):
        if kind == "one":
            lens0 = np.ones(B, np.int32)
            sp = np.concatenate([b for b in special_bags(rows[0], 4, edges)])            # 4 rows at each place, one per bag
            idx0 = np.concatenate([sp, rand0(B - sp.size)])
        elif kind == "fixed":
            lens0 = np.full(B, L_MAX, np.int32)
            sp = special_bags(rows[0], L_MAX, edges)
            idx0 = np.concatenate(sp + [rand0((B - len(sp)) * L_MAX)])
        else:
            lens0 = rng.randint(0, L_MAX + 1, size=B).astype(np.int32)
            sp = special_bags(rows[0], L_MAX, edges)
            lens0[:len(sp)] = [L_MAX, 7, 13, L_MAX, 3, 19][:len(sp)]
            lens0[len(sp):len(sp) + 3] = 0                                               # empty bags
            lens0[-1] = 0
            # (the table's LAST n rows, its first n, and the n rows in the middle of every straddling bag)
            parts = [b[L_MAX - int(n):] if k == 0 else b[:int(n)] if k == 1 else b[(L_MAX - int(n)) // 2:(L_MAX - int(n)) // 2 + int(n)]
                     for k, (b, n) in enumerate(zip(sp, lens0))]
            idx0 = np.concatenate(parts + [rand0(int(lens0[len(sp):].sum()))])
        idx, lens = [idx0], [lens0]
        for t in range(1, T):
            ln = lens0.copy() if kind != "ragged" else rng.randint(0, L_MAX + 1, size=B).astype(np.int32)
            ix = rng.randint(0, rows[t], size=int(ln.sum())).astype(np.int64)
            ix[0], ix[-1] = 0, rows[t] - 1
            idx.append(ix)
            lens.append(ln)
        assert all(int(l.sum()) == i.size for i, l in zip(idx, lens))
        out.append((idx, lens))
    return out


def batches_a(D):
    return batches(ROWS_A, edges_a(D), R_STAR, seed=1000 + D)


def batches_limit(rows):
    """Case B: the last rows, the first, rows around 2^29 (piece offset 2^31 at 4 pieces per row) and random ones"""
    return batches((rows,), (1 << 29,), 1 << 29, seed=77)


def picked_rows(bs, t=0):
    """the distinct rows of table t that the batches name, sorted"""
    return np.unique(np.concatenate([idx[t] for idx, _ in bs]))


# ---- the reference ---------------------------------------------------------------------------------------------------
def fill_rows(picks, D, t, lo, hi, seed):
    """rows `picks` of table t as fill_table_uniform(t, lo, hi, seed) writes them, element by element from the oracle's
    orc_fill_value (element i of a table is a function of (seed, t, i) alone): [len(picks), D] float32.  No array of the whole
    table ever exists."""
    L_ = orc.lib()
    out = np.empty((len(picks), D), np.float32)
    for k, r in enumerate(picks):
        base = int(r) * D
        for c in range(D):
            out[k, c] = L_.orc_fill_value(seed, t, base + c, lo, hi)
    return out


def positions(picks, idx):
    """idx re-indexed into the array of picked rows"""
    pos = np.searchsorted(picks, idx)
    assert np.array_equal(picks[pos], idx)
    return pos.astype(np.int64)
