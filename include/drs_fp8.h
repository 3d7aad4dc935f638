/* drs_fp8.h -- fp8 e4m3 embedding tables ("table_dtype" 4, DRS_TABLE_FP8_E4M3): one entry point of libdrs_hip.so beyond
 * the symbol set of drs.h, which includes this file inside its extern "C" block; do not include it on its own.
 *
 * The symbol set of drs.h is unchanged by it and DRS_ABI_VERSION stays 5: a caller that binds drs.h's list alone (the
 * CPU restatement of the ABI does) sees what it saw before.                                                        */
#ifndef DRS_FP8_H_
#define DRS_FP8_H_

/* The scale exponent k of table t of an fp8 e4m3 arena: the stored code of an element x is e4m3_rne(x * 2^k) (OCP
 * e4m3, round to nearest even, subnormals included -- torch's float8_e4m3fn), a code serves decode(code) * 2^-k.
 *   k is the largest integer with absmax * 2^k <= 448, clamped to [-64, 64], and 0 when absmax is 0: with
 *   absmax = m * 2^e, m in [0.5, 1) (frexp), k = 9 - e if m <= 0.875, else 8 - e.  absmax is the largest |x| over the
 *   table's finite elements -- of the caller's array in drs_set_table, of the source arena's values when "table_dtype" 4
 *   converts loaded fp32 / fp16 / bf16 tables (an int8 / int4 rowwise arena refuses 4: DRS_ERR_BAD_ARG).
 *   drs_fill_table_uniform takes absmax = max(|lo|, |hi|) without looking at the samples, so its k may be one less
 *   than the conversion of the same fp32 fill would pick.
 *   A NaN or infinite element is stored as an e4m3 NaN (0x7F, with the element's sign bit) and serves NaN.
 * DRS_ERR_UNSUPPORTED unless the arena in use is fp8; DRS_ERR_BAD_ARG for a bad table id or a null k.             */
int32_t drs_table_fp8_exponent(drs_handle h, int32_t t, int32_t* k);

#endif /* DRS_FP8_H_ */
