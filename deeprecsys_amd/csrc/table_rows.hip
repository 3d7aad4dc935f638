// Single rows of a loaded table (drs_update_rows / drs_get_rows, engine_rows.hip): the one pass table_convert.hip lacks, rows
// moved between a packed buffer and the table rows an id list names.  Everything that gives a row its stored bytes or its
// served value stays table_convert.hip's: an update converts the caller's fp32 rows into a packed buffer of the table's type
// with the kernels drs_set_table runs (launch_convert_rows) and this pass places them; a read-back packs the named rows
// and write_elems_kernel widens them.  So an updated row holds drs_set_table's bytes by construction.
#include "drs_internal.h"

namespace drs {

// One wave per row, four rows per workgroup: row r of `buf` (r * S bytes in) <-> row ids[r] of the table at `table`, whose
// rows lie where i8_row_offset puts them (n: I8Lines::n of a line-packed rowwise table, 0: every other layout, ids[r] * S
// -- all in 64 bits: a row may lie beyond byte 2^32 of its table).  A wave touches the S bytes of its own row and nothing
// else: the neighbours in a 128-byte line and the line's zero tail keep their bytes.  W: the unit moved, 4 bytes when S is
// a multiple of 4 (every shipped shape), else 1.  The caller passes distinct ids when it writes the table.
template <class W>
__global__ __launch_bounds__(256) void move_rows_kernel(uint8_t* buf, uint8_t* table, const int64_t* ids, int64_t rows, int S, int32_t n, int to_table) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
    uint8_t* packed = buf + r * S;
    uint8_t* stored = table + i8_row_offset(ids[r], S, n);
    const uint8_t* from = to_table ? packed : stored;
    uint8_t* to = to_table ? stored : packed;
    for (int c = lane * (int)sizeof(W); c < S; c += 64 * (int)sizeof(W)) *reinterpret_cast<W*>(to + c) = *reinterpret_cast<const W*>(from + c);
  }
}

hipError_t launch_move_rows(void* buf, void* table, const int64_t* d_ids, int64_t rows, int64_t S, int32_t lines_n, bool to_table, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (S <= 0 || S > (1 << 20)) return hipErrorInvalidValue;
  const int64_t want = (rows + 3) / 4;
  const dim3 grid((unsigned)(want < 16384 ? want : 16384)), block(256);
  uint8_t* b = static_cast<uint8_t*>(buf);
  uint8_t* t = static_cast<uint8_t*>(table);
  if (S % 4 == 0) hipLaunchKernelGGL(move_rows_kernel<uint32_t>, grid, block, 0, s, b, t, d_ids, rows, (int)S, lines_n, (int)to_table);
  else hipLaunchKernelGGL(move_rows_kernel<uint8_t>, grid, block, 0, s, b, t, d_ids, rows, (int)S, lines_n, (int)to_table);
  return hipGetLastError();
}

}  // namespace drs
