/* drs_rows.h -- single rows of a loaded embedding table, written and read back in whatever type the table is stored:
 * two entry points of libdrs_hip.so beyond the symbol set of drs.h, which includes this file inside its extern "C" block;
 * do not include it on its own.
 *
 * FBGEMM's inference tables have emb_inplace_update for the same purpose: a deployed recommender refreshes rows all the
 * time, and drs_set_table uploads and converts a whole table.  The symbol set of drs.h is unchanged by them and
 * DRS_ABI_VERSION stays 5: a caller that binds drs.h's list alone (the CPU restatement of the ABI does) sees what it saw
 * before.                                                                                                              */
#ifndef DRS_ROWS_H_
#define DRS_ROWS_H_

/* Row h_ids[i] of table t becomes what drs_set_table would have stored for a row holding h_V[i], in the arena's current
 * "table_dtype" and line layout: fp32 the bits given; fp16 / bf16 rounded to nearest even; int8 / int4 rowwise the row
 * quantized on its own (embedding_bag_byte_prepack / embedding_bag_4bit_prepack of that row, byte for byte), placed by
 * the plain or the line-packed row map -- the other rows of its 128-byte line and the line's zero tail keep their bytes;
 * fp8 e4m3 e4m3_rne(x * 2^k_t) under the table's EXISTING k_t.  An fp8 update never re-derives the scale: a finite
 * element with |x| * 2^k_t > 448 is DRS_ERR_BAD_ARG (set the whole table again with drs_set_table); NaN and +-inf are
 * stored as drs_set_table stores them.
 *   Synchronous: drains the engine first (drs_sync), as drs_set_table does -- a launch set already enqueued is served
 *   from the old rows, every later one from the new ones -- and drops the other placement candidates likewise.
 *   Duplicate ids are legal, the LAST occurrence wins.  n == 0: DRS_OK, nothing done.  All six model kinds.
 *   DRS_ERR_BAD_ARG: a bad table id, n < 0, a null pointer with n > 0, a table that was never set or filled;
 *   DRS_ERR_INDEX_RANGE: an id outside [0, rows_t).  Every id and value is checked before the first write: a refused
 *   call changes nothing.                                                                                            */
int32_t drs_update_rows(drs_handle h, int32_t t, int64_t n, const int64_t* h_ids /*[n]*/, const float* h_V /*[n, D]*/);

/* h_V[i] receives the fp32 value row h_ids[i] of table t serves as a one-row bag: fp32 the stored bits, fp16 / bf16 the
 * widened value, int8 / int4 rowwise fmaf(scale, q, 0.0f + bias), fp8 decode(code) * 2^-k_t.  Ids in any order,
 * duplicates allowed.  Drains the engine first; the refusals of drs_update_rows.                                      */
int32_t drs_get_rows(drs_handle h, int32_t t, int64_t n, const int64_t* h_ids /*[n]*/, float* h_V /*[n, D]*/);

#endif /* DRS_ROWS_H_ */
