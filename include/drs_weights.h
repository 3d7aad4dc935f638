/* drs_weights.h -- per-sample weights (SparseLengthsWeightedSum): two entry points of libdrs_hip.so beyond the symbol
 * set of drs.h, which includes this file inside its extern "C" block; do not include it on its own.
 *
 * Caffe2 has SparseLengthsWeightedSum([tbl, w, idx, len]); torch has EmbeddingBag(mode="sum", per_sample_weights=),
 * and its quantized embedding_bag_*_rowwise_offsets(per_sample_weights=) are the same operator on rowwise tables.
 * The symbol set of drs.h is unchanged by them and DRS_ABI_VERSION stays 5: a caller that binds drs.h's list alone
 * (the CPU restatement of the ABI does) sees what it saw before.                                                   */
#ifndef DRS_WEIGHTS_H_
#define DRS_WEIGHTS_H_

/* Per-sample weights (SparseLengthsWeightedSum([tbl, w, idx, len]); torch's EmbeddingBag(mode="sum",
 * per_sample_weights=)) for a batch that is ALREADY staged: h_wgt[t][j] weighs index j of table t, and a bag's pooled
 * vector becomes the chain acc = fma(w_j, row_j, acc) in index order (rowwise tables: s = w * scale, b = w * bias,
 * acc = fma(s, q, acc + b)) -- under "sls_exact" 1 bit-identical to torch's CPU operators; otherwise the same
 * per-row step in the split order.  n_idx[t] must be what drs_stage_batch staged for table t (DRS_ERR_LENGTHS_SUM
 * otherwise, nothing changes); a NULL h_wgt[t] gives every index of table t the weight 1.0f (n_idx[t] is not read
 * then).  drs_stage_batch on the same batch_id drops the weights: the batch is unweighted again.  Non-finite
 * weights are outside the contract, as non-finite table values are.  drs_forward, drs_forward_async and
 * drs_forward_multi_async serve weighted batches, also mixed with unweighted ones in one launch set (an unweighted
 * query keeps its sequential bits there); the host per-call input paths (drs_forward_inputs*, drs_run_queues*)
 * carry no weights, the device-array ones carry them through drs_device_weights.h.  A launch set with a weighted query takes the ring walk or the any-width form, never the flat or
 * one-lookup forms (dispatch log: a "w" token).  DIN and DIEN: DRS_ERR_UNSUPPORTED; so is a handle under "sls_pool" 1
 * (there is no weighted mean), and "sls_pool" 1 is refused while a staged batch carries weights.  drs_gather_bytes
 * counts 4 more bytes per looked-up row of a weighted batch.  Read-only option "sls_weighted": staged batches that
 * carry weights.  (Added without an ABI version change: nothing existing moved.)                                  */
int32_t drs_stage_batch_weights(drs_handle h, int32_t batch_id,
                                const float* const* h_wgt /*[T] -> [n_idx[t]] or NULL*/,
                                const int64_t* n_idx /*[T]*/);

/* drs_sls_weighted == SparseLengthsWeightedSum([tbl, w, idx, len]): d_wgt[j] weighs d_idx[j];
 *   out[b,:] = the chain acc = fma(w, W[idx,:], acc) over the bag's indices, in index order when
 *   exact_order != 0 (bit-identical to torch's CPU embedding_bag(per_sample_weights=)); fp32 tables, like
 *   drs_sls; an out-of-range index is DRS_ERR_INDEX_RANGE and contributes nothing.  Refused under the
 *   handle's "sls_pool" 1 (DRS_ERR_UNSUPPORTED).                                                       */
int32_t drs_sls_weighted(drs_handle h, const float* d_W, int64_t rows, int32_t D,
                         const int32_t* d_idx, const float* d_wgt, const int32_t* d_len,
                         int64_t n_bags, int64_t n_idx, float* d_out /*[n_bags, D]*/, int32_t exact_order);

#endif /* DRS_WEIGHTS_H_ */
