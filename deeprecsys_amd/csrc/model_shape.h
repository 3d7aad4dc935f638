// The shape algebra of the reference's model builders, per model kind: from a drs_model_cfg to the widths drs_create lays the
// engine out by, or the builder's refusal (the reference's sys.exit checks: models/dlrm_s_caffe2.py:432-440).  Plain C++ over
// include/drs.h alone, so that a host program can include it on its own (tests/test_model_shape_cpu.py).  What needs the
// kernels' word -- whether a DIN unit or a DIEN layer fits the LDS (din.hip, dien.hip) -- stays in drs_create.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/drs.h"

namespace drs {
namespace eng {

struct MlpShape {
  std::vector<int32_t> ln;     // the widths, input first; ln.size() - 1 layers
  int32_t sigmoid_layer = -1;  // 1-based, -1 none
};

struct ModelShape {
  int32_t code = DRS_OK;       // not DRS_OK: the refusal, nothing else is to be read
  const char* msg = nullptr;
  int32_t m_den = 0, w0 = 0;   // dense input width, dense_out width
  int32_t num_int = 0, n_out = 0;
  MlpShape bot, top, fin;
  MlpShape task;               // MT-WnD: one of the n_tasks equal task heads
  int32_t n_tasks = 0;
  MlpShape att;                // DIN: one of the n_att equal attention units
  int32_t n_att = 0;
  std::vector<MlpShape> rnn;   // DIEN: the two BasicRNN layers, each {i2h, gates_t}
  bool din_any = false;        // DIN: units din.hip has no form for (depth != 2, wide hidden layer, D not 4 k <= 256) -> din_any.hip
  int din_maxw = 0;            // ... their widest hidden layer
};

// cfg as drs_create has vetted it so far: non-null arrays, num_tables >= 1, n_bot >= 1, n_top >= 2, sparse_dim in [1, 4096]
inline ModelShape model_shape(const drs_model_cfg& cfg) {
  ModelShape m;
  auto refuse = [&m](int32_t code, const char* msg) { m.code = code; m.msg = msg; return m; };
  const int D = cfg.sparse_dim, T = cfg.num_tables, F = T + 1;
  m.bot.ln.assign(cfg.ln_bot, cfg.ln_bot + cfg.n_bot);
  m.top.ln.assign(cfg.ln_top, cfg.ln_top + cfg.n_top);
  // (only DLRM's and W&D's top MLP ends in the sigmoid; NCF's output width arrives with its predictor)
  const bool sig = cfg.model_kind == DRS_MODEL_DLRM || cfg.model_kind == DRS_MODEL_WND;
  m.top.sigmoid_layer = sig ? cfg.sigmoid_top : -1;
  m.n_out = m.top.ln.back();
  switch (cfg.model_kind) {
    case DRS_MODEL_DLRM: {
      m.m_den = m.bot.ln.front();
      m.w0 = m.bot.ln.back();
      if (m.w0 != D) return refuse(DRS_ERR_BAD_ARG, "arch_sparse_feature_size does not match last dim of bottom mlp");
      const bool itself = cfg.interaction_itself != 0;
      if (cfg.interaction_op == DRS_INTERACT_DOT)
        m.num_int = (itself ? F * (F + 1) / 2 : F * (F - 1) / 2) + D;
      else if (cfg.interaction_op == DRS_INTERACT_CAT)
        m.num_int = F * D;
      else
        return refuse(DRS_ERR_BAD_ARG, "unknown interaction op");
      if (m.num_int != m.top.ln.front()) return refuse(DRS_ERR_BAD_ARG, "# of feature interactions does not match first dim of top mlp");
      break;
    }
    case DRS_MODEL_WND:
    case DRS_MODEL_MTWND: {
      const bool mt = cfg.model_kind == DRS_MODEL_MTWND;
      if (cfg.n_bot != 1) return refuse(DRS_ERR_BAD_ARG, mt ? "MT-W&D has no bottom MLP layers" : "W&D has no bottom MLP layers");
      m.m_den = m.w0 = m.bot.ln.front();
      m.num_int = T * D + m.w0;
      if (m.num_int != m.top.ln.front()) return refuse(DRS_ERR_BAD_ARG, "num_int does not match first dim of top mlp");
      if (!mt) break;
      if (cfg.n_task < 2 || !cfg.ln_task || cfg.num_tasks < 1 || cfg.num_tasks > 64)
        return refuse(DRS_ERR_BAD_ARG, "MT-W&D needs arch_mlp_tasks and 1..64 task heads");
      if (cfg.ln_task[0] != m.top.ln.back())
        return refuse(DRS_ERR_BAD_ARG, "Shared top layer and task MLP layers must have same input/output dimension");
      m.n_tasks = cfg.num_tasks;
      m.task.ln.assign(cfg.ln_task, cfg.ln_task + cfg.n_task);
      m.task.sigmoid_layer = cfg.sigmoid_top;    // multi_task_wnd.py:309 passes self.sigmoid_top to the heads (:301: the top gets -1)
      m.n_out = cfg.num_tasks * cfg.ln_task[cfg.n_task - 1];
      break;
    }
    case DRS_MODEL_DIN: {
      if (T < 4) return refuse(DRS_ERR_BAD_ARG, "DIN needs at least 4 embedding tables");
      // an attention unit is create_mlp over 3*D - <arch_mlp_bot> - D (models/din.py:255-277): any depth, any widths
      if (cfg.n_bot < 2 || m.bot.ln.front() != 3 * D || m.bot.ln.back() != D)
        return refuse(DRS_ERR_BAD_ARG, "DIN attention unit must be 3*D -> ... -> D");
      for (int w : m.bot.ln) if (w < 1) return refuse(DRS_ERR_BAD_ARG, "DIN attention unit with an empty layer");
      // din.hip's forms: one hidden layer of <= 64 units, rows in 16-byte pieces; the two-launch attention kernel (the only
      // path for sls_exact = 1 and for shapes the fused launch is not instantiated for) keeps 4 samples x (T - 3) units x
      // h hidden values in 64 KB of LDS.  Everything else: din_any.hip.
      m.din_any = cfg.n_bot != 3 || m.bot.ln[1] > 64 || (int64_t)(T - 3) * m.bot.ln[1] > 4096 || (D & 3) || D > 256;
      for (int l = 1; l + 1 < cfg.n_bot; ++l) m.din_maxw = std::max(m.din_maxw, m.bot.ln[l]);
      m.num_int = 4 * D;
      if (m.num_int != m.top.ln.front()) return refuse(DRS_ERR_BAD_ARG, "# of feature interactions does not match first dim of top mlp");
      m.n_att = T - 3;
      m.att.ln = m.bot.ln;
      m.bot.ln = {0};                            // no bottom MLP of its own
      break;
    }
    case DRS_MODEL_DIEN: {
      if (T < 4) return refuse(DRS_ERR_BAD_ARG, "DIEN needs at least 4 embedding tables");
      if (cfg.n_bot != 2 || m.bot.ln[0] != D || m.bot.ln[1] < 1) return refuse(DRS_ERR_BAD_ARG, "DIEN: ln_bot must be [D, hidden_size]");
      const int H = m.bot.ln[1];
      m.num_int = H + 3 * D;
      if (m.num_int != m.top.ln.front()) return refuse(DRS_ERR_BAD_ARG, "# of feature interactions does not match first dim of top mlp");
      m.rnn.resize(2);
      m.rnn[0].ln = {D, H, H};
      m.rnn[1].ln = {H, H, H};
      m.bot.ln = {0};
      break;
    }
    case DRS_MODEL_NCF: {
      if (T != 4) return refuse(DRS_ERR_BAD_ARG, "NCF has 4 embedding tables");
      if (m.top.ln.front() != 2 * D) return refuse(DRS_ERR_BAD_ARG, "NCF MLP branch input must be 2*D");
      m.num_int = D + m.top.ln.back();
      m.fin.ln = {m.num_int, 0};  // output width arrives with drs_set_fc(DRS_MLP_FINAL)
      m.n_out = 0;
      break;
    }
    default:
      return refuse(DRS_ERR_BAD_ARG, "unknown model kind");
  }
  for (int t = 0; t < T; ++t) {
    if (cfg.table_rows[t] <= 0) return refuse(DRS_ERR_BAD_ARG, "table with no rows");
    // row offsets travel as 32-bit counts of load-width units (8 or 16 bytes): 32 GiB per table
    if (cfg.table_rows[t] * (int64_t)D >= (1ll << 33)) return refuse(DRS_ERR_UNSUPPORTED, "rows*D must be < 2^33 per table");
  }
  // prefix sums and bag * length products are int32 on the device
  if ((int64_t)cfg.max_batch * cfg.max_lookups >= (1ll << 31) / DRS_MAX_COALESCE)
    return refuse(DRS_ERR_UNSUPPORTED, "max_batch * max_lookups must stay below 2^31 / 8");
  return m;
}

}  // namespace eng
}  // namespace drs
