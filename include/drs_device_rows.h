/* drs_device_rows.h -- single rows of a loaded embedding table, updated and read back from DEVICE arrays: two entry points of
 * libdrs_hip.so beyond the symbol set of drs.h, which includes this file inside its extern "C" block; do not include it on
 * its own.
 *
 * drs_update_rows / drs_get_rows (drs_rows.h) take host ids and host fp32 rows.  A trainer or feature pipeline that produces
 * refreshed rows on the engine's GPU had to synchronise its stream, download n ids and n * D floats, let the host check, sort
 * and scan them, and let the engine upload them again.  Here the ids and the rows stay where they are: the range check, the
 * last-wins de-duplication and the fp8 fit check are kernel passes (csrc/device_rows.hip, csrc/row_dedup.h), the stored
 * bytes are made by the kernels drs_set_table runs.  The symbol set of drs.h is unchanged and DRS_ABI_VERSION stays 5.   */
#ifndef DRS_DEVICE_ROWS_H_
#define DRS_DEVICE_ROWS_H_

/* the most rows one call names (2^24): the de-duplication table of a call holds 16 bytes per named row */
#define DRS_DEVICE_ROWS_MAX ((int64_t)1 << 24)

/* Row d_ids[i] of table t becomes exactly what drs_update_rows would have stored for the same ids and the same values
 * widened to fp32 -- in every stored type ("table_dtype" 0, 1, 2, 4, 8, 9) and both line layouts; fp8 under the table's
 * EXISTING scale; the other rows of a 128-byte line and the line's zero tail keep their bytes.  Duplicate ids are legal, the
 * LAST occurrence wins.  n == 0: DRS_OK, nothing done.  All six model kinds.
 *
 * d_ids   [n] int64, contiguous, 8-byte aligned.
 * d_V     [n, D] elements of val_dtype -- DRS_TABLE_FP32, DRS_TABLE_FP16 or DRS_TABLE_BF16 --, rows val_row_stride ELEMENTS
 *         apart, the pointer aligned to its element, no more.  val_row_stride >= D where n > 1 (a column block of a wider
 *         tensor goes down as it is); the stride of a single row is not read.  Widening is exact: fp16 / bf16 values give the
 *         rows their widened values give as fp32.
 * Ordering.  ordered == 0: the arrays are complete when the call is made; `stream` is ignored.  ordered == 1: the engine
 *         records an event on `stream` (a hipStream_t; NULL is HIP's null stream and is valid) and its passes wait for it,
 *         so the caller does not synchronise the work that produces the arrays.  In both forms the call is drs_update_rows'
 *         twin towards the engine: it drains the engine first (drs_sync) -- a launch set already enqueued is served from the
 *         old rows, every later one from the new ones -- and drops the other placement candidates.  It returns its status
 *         only after its own passes have finished on the device: work the caller enqueues after the call has returned sees
 *         the new rows.  (An update that neither drains nor waits on the host is not offered.)
 * Refused before anything is enqueued, DRS_ERR_BAD_ARG: a bad table id, n < 0, a table that was never set or filled;
 *         `ordered` outside {0, 1}; a val_dtype outside the three; and, with n > 0: a null pointer; n > DRS_DEVICE_ROWS_MAX; a
 *         pointer not aligned to its element type; val_row_stride < D with n > 1, or an extent -- (n - 1) * val_row_stride + D
 *         elements -- beyond 2^60 bytes; d_ids or d_V failing the pointer check of drs_device_inputs.h (plain device memory of
 *         the engine's GPU whose extent ends inside its allocation; hipMemGetAddressRange).
 * Found on the device and returned by the call itself: DRS_ERR_INDEX_RANGE, an id outside [0, rows_t) -- tested on the 64-bit
 *         value, before any narrowing; DRS_ERR_BAD_ARG, a finite value with |x| * 2^k_t > 448 under fp8.  drs_last_error
 *         names the lowest offending position.  No id is used as a row before it is checked: bad arrays cost an error code,
 *         never a fault.  A refused call changes nothing.                                                                 */
int32_t drs_update_rows_device(drs_handle h, int32_t t, int64_t n, const int64_t* d_ids /*[n], contiguous*/,
                               const void* d_V /*[n, D]*/, int64_t val_row_stride /*elements*/, int32_t val_dtype,
                               void* stream /*hipStream_t*/, int32_t ordered);

/* d_V[i] receives what drs_get_rows returns for row d_ids[i]: the fp32 value the row serves as a one-row bag.  Exactly the
 * n * D floats are written, nothing between rows val_row_stride floats apart.  Ids in any order, duplicates allowed.
 * Ordering, refusals and device-found errors as above (values are not checked: there are none); a failed call writes
 * nothing to d_V.  When the call has returned, d_V is complete: work enqueued afterwards on any stream reads the rows.     */
int32_t drs_get_rows_device(drs_handle h, int32_t t, int64_t n, const int64_t* d_ids, float* d_V /*[n, D] fp32*/,
                            int64_t val_row_stride /*floats*/, void* stream, int32_t ordered);

#endif /* DRS_DEVICE_ROWS_H_ */
