"""csrc/model_shape.h on its own, in a host program: the per-model shape algebra drs_create starts from.  For the six model
kinds the configs are the ones dlrm_s_hip.py builds from the golden fixtures' arguments, and the derived widths are the
ones DESIGN.md and dlrm_s_hip.py state; every refusal is reached once and its code and exact text pinned.  Built with the
host sanitizers and once without them."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deeprecsys_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")

KIND = {"dlrm": "DRS_MODEL_DLRM", "wnd": "DRS_MODEL_WND", "ncf": "DRS_MODEL_NCF", "mtwnd": "DRS_MODEL_MTWND", "din": "DRS_MODEL_DIN",
        "dien": "DRS_MODEL_DIEN"}
CASES = ["dlrm_dot_small", "dlrm_rm1_mini", "wnd_mini", "mtwnd_mini", "ncf_mini", "din_mini", "dien_mini"]


def ints(s):
    return [int(x) for x in str(s).split("-")]


def case_of(name):
    """(the drs_model_cfg dlrm_s_hip.py's net classes hand to the engine, the widths the engine must derive from it), both
    from the fixture's arguments by the reference's own arithmetic"""
    a = json.load(open(os.path.join(GOLDEN, name + ".json")))["args"]
    kind, D, rows = a["model_type"], int(a["arch_sparse_feature_size"]), ints(a["arch_embedding_size"])
    T = len(rows)
    cfg = dict(kind=kind, rows=rows, D=D, op="DRS_INTERACT_CAT", itself=0, sigmoid_top=-1, ln_task=[], num_tasks=0)
    exp = dict(m_den=0, w0=0, n_tasks=0, n_att=0, n_rnn=0, fin=[], task=[], att=[], bot=[0], top_sigmoid=-1, task_sigmoid=-1,
               din_any=0, din_maxw=0, rnn=[[], []])
    if kind == "dlrm":
        bot, F = ints(a["arch_mlp_bot"]), T + 1
        dot = a["arch_interaction_op"] == "dot"
        itself = bool(a["arch_interaction_itself"])
        num_int = (F * (F + 1) // 2 if itself else F * (F - 1) // 2) + bot[-1] if dot else F * bot[-1]
        top = [num_int] + ints(a["arch_mlp_top"])
        cfg.update(bot=bot, top=top, op="DRS_INTERACT_DOT" if dot else "DRS_INTERACT_CAT", itself=int(itself), sigmoid_top=len(top) - 1)
        exp.update(m_den=bot[0], w0=bot[-1], num_int=num_int, n_out=top[-1], bot=bot, top=top, top_sigmoid=len(top) - 1)
    elif kind in ("wnd", "mtwnd"):
        bot = ints(a["arch_mlp_bot"])
        num_int = T * D + bot[0]
        top = [num_int] + ints(a["arch_mlp_top"])
        cfg.update(bot=bot, top=top, sigmoid_top=len(top) - 1)
        exp.update(m_den=bot[0], w0=bot[0], num_int=num_int, n_out=top[-1], bot=bot, top=top, top_sigmoid=len(top) - 1)
        if kind == "mtwnd":
            task, n = ints(a["arch_mlp_tasks"]), int(a["num_multi_tasks"])
            cfg.update(ln_task=task, num_tasks=n)
            exp.update(n_out=n * task[-1], n_tasks=n, task=task, top_sigmoid=-1, task_sigmoid=len(top) - 1)
    elif kind == "ncf":
        top = ([2 * D] + ints(a["arch_mlp_top"]))[:-1]         # the predictor is DRS_MLP_FINAL, its width arrives with its weights
        cfg.update(bot=[0], top=top)
        exp.update(num_int=D + top[-1], n_out=0, top=top, fin=[D + top[-1], 0])
    elif kind == "din":
        att = [3 * D] + ints(a["arch_mlp_bot"]) + [D]
        top = [4 * D] + ints(a["arch_mlp_top"])
        cfg.update(bot=att, top=top)
        hidden = att[1:-1]
        any_ = len(att) != 3 or att[1] > 64 or (T - 3) * att[1] > 4096 or D % 4 != 0 or D > 256
        exp.update(num_int=4 * D, n_out=top[-1], top=top, n_att=T - 3, att=att, din_any=int(any_), din_maxw=max(hidden))
    elif kind == "dien":
        Hs = int(a["hidden_size"])
        top = [Hs + 3 * D] + ints(a["arch_mlp_top"])
        cfg.update(bot=[D, Hs], top=top)
        exp.update(num_int=Hs + 3 * D, n_out=top[-1], top=top, n_rnn=2, rnn=[[D, Hs, Hs], [Hs, Hs, Hs]])
    return cfg, exp


def braces(v):
    return "{" + ", ".join(str(x) for x in v) + "}"


def render(name):
    c, e = case_of(name)
    return ('  {"%s", %s, %s, %d, %s, %s, %s, %d, %d, %s, %d,\n   %d, %d, %d, %d, %s, %s, %d, %s, %s, %d, %d, %s, %d, %d, %d, %d, %s, %s},'
            % (name, KIND[c["kind"]], braces(c["rows"]), c["D"], braces(c["bot"]), braces(c["top"]), c["op"], c["itself"], c["sigmoid_top"],
               braces(c["ln_task"]), c["num_tasks"],
               e["m_den"], e["w0"], e["num_int"], e["n_out"], braces(e["bot"]), braces(e["top"]), e["top_sigmoid"], braces(e["fin"]),
               braces(e["task"]), e["task_sigmoid"], e["n_tasks"], braces(e["att"]), e["n_att"], e["din_any"], e["din_maxw"], e["n_rnn"],
               braces(e["rnn"][0]), braces(e["rnn"][1])))


SHAPE_MAIN = r"""
#include "model_shape.h"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace drs::eng;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (++fails < 40) printf("line %d: %s\n", __LINE__, #c); } } while (0)
typedef std::vector<int32_t> V;

struct Cfg {
  int32_t kind;
  std::vector<int64_t> rows;
  int32_t D;
  V bot, top;
  int32_t op, itself, sigmoid_top;
  V task;
  int32_t num_tasks;
  int32_t max_batch = 64, max_lookups = 4;
  drs_model_cfg c() const {
    drs_model_cfg m;
    memset(&m, 0, sizeof m);
    m.model_kind = kind; m.num_tables = (int32_t)rows.size(); m.table_rows = rows.data(); m.sparse_dim = D;
    m.n_bot = (int32_t)bot.size(); m.ln_bot = bot.data(); m.n_top = (int32_t)top.size(); m.ln_top = top.data();
    m.interaction_op = op; m.interaction_itself = itself; m.sigmoid_top = sigmoid_top;
    m.max_batch = max_batch; m.max_lookups = max_lookups; m.num_staged_batches = 1; m.num_slots = 2;
    m.n_task = (int32_t)task.size(); m.ln_task = task.empty() ? nullptr : task.data(); m.num_tasks = num_tasks;
    return m;
  }
};

// ---- the fixtures' shapes ----
struct Case {
  const char* name;
  int32_t kind; std::vector<int64_t> rows; int32_t D; V bot, top; int32_t op, itself, sigmoid_top; V task; int32_t num_tasks;
  int32_t m_den, w0, num_int, n_out; V e_bot, e_top; int32_t top_sigmoid; V fin, e_task; int32_t task_sigmoid, n_tasks; V att;
  int32_t n_att, din_any, din_maxw, n_rnn; V rnn0, rnn1;
};
static const Case CASES[] = {
@CASES@
};
static void fixtures() {
  for (const Case& k : CASES) {
    const Cfg cfg{k.kind, k.rows, k.D, k.bot, k.top, k.op, k.itself, k.sigmoid_top, k.task, k.num_tasks};
    const ModelShape m = model_shape(cfg.c());
    const int before = fails;
    CHECK(m.code == DRS_OK && m.msg == nullptr);
    CHECK(m.m_den == k.m_den && m.w0 == k.w0 && m.num_int == k.num_int && m.n_out == k.n_out);
    CHECK(m.bot.ln == k.e_bot && m.top.ln == k.e_top && m.top.sigmoid_layer == k.top_sigmoid && m.bot.sigmoid_layer == -1);
    CHECK(m.fin.ln == k.fin && m.fin.sigmoid_layer == -1);
    CHECK(m.n_tasks == k.n_tasks && m.task.ln == k.e_task && m.task.sigmoid_layer == k.task_sigmoid);
    CHECK(m.n_att == k.n_att && m.att.ln == k.att && m.att.sigmoid_layer == -1);
    CHECK((int)m.din_any == k.din_any && m.din_maxw == k.din_maxw);
    CHECK((int)m.rnn.size() == k.n_rnn);
    if (m.rnn.size() == 2) CHECK(m.rnn[0].ln == k.rnn0 && m.rnn[1].ln == k.rnn1 && m.rnn[0].sigmoid_layer == -1 && m.rnn[1].sigmoid_layer == -1);
    if (fails != before) printf("  ... in %s\n", k.name);
  }
}

// ---- every refusal, once: the code and the exact text ----
static void refused(const Cfg& cfg, int32_t code, const char* msg, int line) {
  const ModelShape m = model_shape(cfg.c());
  if (m.code != code || !m.msg || strcmp(m.msg, msg)) {
    ++fails;
    printf("line %d: code %d \"%s\", expected %d \"%s\"\n", line, m.code, m.msg ? m.msg : "(none)", code, msg);
  }
}
#define REFUSED(cfg, code, msg) refused(cfg, code, msg, __LINE__)
static void refusals() {
  const char* kTop = "# of feature interactions does not match first dim of top mlp";
  // T = 3, D = 8: cat interaction of 4 features
  const Cfg dlrm{DRS_MODEL_DLRM, {10, 20, 30}, 8, {4, 8}, {32, 4, 1}, DRS_INTERACT_CAT, 0, 2, {}, 0};
  CHECK(model_shape(dlrm.c()).code == DRS_OK);
  Cfg c = dlrm; c.bot = {4, 6};
  REFUSED(c, DRS_ERR_BAD_ARG, "arch_sparse_feature_size does not match last dim of bottom mlp");
  c = dlrm; c.op = 7;
  REFUSED(c, DRS_ERR_BAD_ARG, "unknown interaction op");
  c = dlrm; c.top = {33, 4, 1};
  REFUSED(c, DRS_ERR_BAD_ARG, kTop);
  c = dlrm; c.op = DRS_INTERACT_DOT;                      // 4 * 3 / 2 + 8 = 14, not 32 ...
  REFUSED(c, DRS_ERR_BAD_ARG, kTop);
  c.top = {14, 4, 1};
  CHECK(model_shape(c.c()).num_int == 14);
  c.itself = 1;                                           // ... and 4 * 5 / 2 + 8 = 18 with the diagonal
  REFUSED(c, DRS_ERR_BAD_ARG, kTop);
  c.top = {18, 4, 1};
  CHECK(model_shape(c.c()).num_int == 18);
  c = dlrm; c.kind = 6;
  REFUSED(c, DRS_ERR_BAD_ARG, "unknown model kind");
  c = dlrm; c.rows = {10, 0, 30};
  REFUSED(c, DRS_ERR_BAD_ARG, "table with no rows");
  c = dlrm; c.rows = {10, (int64_t)1 << 30, 30};          // rows * D = 2^33
  REFUSED(c, DRS_ERR_UNSUPPORTED, "rows*D must be < 2^33 per table");
  c.rows = {10, ((int64_t)1 << 30) - 1, 30};
  CHECK(model_shape(c.c()).code == DRS_OK);
  c = dlrm; c.max_batch = (int32_t)((1ll << 31) / DRS_MAX_COALESCE / 4); c.max_lookups = 4;   // the product is the bound itself
  REFUSED(c, DRS_ERR_UNSUPPORTED, "max_batch * max_lookups must stay below 2^31 / 8");
  c.max_lookups = 3;
  CHECK(model_shape(c.c()).code == DRS_OK);

  const Cfg wnd{DRS_MODEL_WND, {10, 20, 30}, 8, {5}, {29, 4, 1}, DRS_INTERACT_CAT, 0, 2, {}, 0};
  CHECK(model_shape(wnd.c()).code == DRS_OK);
  c = wnd; c.bot = {5, 8};
  REFUSED(c, DRS_ERR_BAD_ARG, "W&D has no bottom MLP layers");
  c = wnd; c.top = {28, 4, 1};
  REFUSED(c, DRS_ERR_BAD_ARG, "num_int does not match first dim of top mlp");

  const Cfg mt{DRS_MODEL_MTWND, {10, 20, 30}, 8, {5}, {29, 6, 4}, DRS_INTERACT_CAT, 0, 2, {4, 2, 1}, 3};
  CHECK(model_shape(mt.c()).code == DRS_OK && model_shape(mt.c()).n_out == 3);
  c = mt; c.bot = {5, 8};
  REFUSED(c, DRS_ERR_BAD_ARG, "MT-W&D has no bottom MLP layers");
  c = mt; c.top = {30, 6, 4};
  REFUSED(c, DRS_ERR_BAD_ARG, "num_int does not match first dim of top mlp");
  c = mt; c.task = {4};
  REFUSED(c, DRS_ERR_BAD_ARG, "MT-W&D needs arch_mlp_tasks and 1..64 task heads");
  c = mt; c.task = {};
  REFUSED(c, DRS_ERR_BAD_ARG, "MT-W&D needs arch_mlp_tasks and 1..64 task heads");
  c = mt; c.num_tasks = 0;
  REFUSED(c, DRS_ERR_BAD_ARG, "MT-W&D needs arch_mlp_tasks and 1..64 task heads");
  c = mt; c.num_tasks = 65;
  REFUSED(c, DRS_ERR_BAD_ARG, "MT-W&D needs arch_mlp_tasks and 1..64 task heads");
  c = mt; c.task = {5, 2, 1};
  REFUSED(c, DRS_ERR_BAD_ARG, "Shared top layer and task MLP layers must have same input/output dimension");

  const Cfg din{DRS_MODEL_DIN, {10, 20, 30, 40, 50}, 8, {24, 6, 8}, {32, 4, 1}, DRS_INTERACT_CAT, 0, -1, {}, 0};
  CHECK(model_shape(din.c()).code == DRS_OK && !model_shape(din.c()).din_any && model_shape(din.c()).n_att == 2);
  c = din; c.rows = {10, 20, 30};
  REFUSED(c, DRS_ERR_BAD_ARG, "DIN needs at least 4 embedding tables");
  c = din; c.bot = {24};
  REFUSED(c, DRS_ERR_BAD_ARG, "DIN attention unit must be 3*D -> ... -> D");
  c = din; c.bot = {23, 6, 8};
  REFUSED(c, DRS_ERR_BAD_ARG, "DIN attention unit must be 3*D -> ... -> D");
  c = din; c.bot = {24, 6, 7};
  REFUSED(c, DRS_ERR_BAD_ARG, "DIN attention unit must be 3*D -> ... -> D");
  c = din; c.bot = {24, 0, 8};
  REFUSED(c, DRS_ERR_BAD_ARG, "DIN attention unit with an empty layer");
  c = din; c.top = {31, 4, 1};
  REFUSED(c, DRS_ERR_BAD_ARG, kTop);
  c = din; c.bot = {24, 6, 5, 8};                         // two hidden layers: the any-shape form, widest hidden layer 6
  CHECK(model_shape(c.c()).code == DRS_OK && model_shape(c.c()).din_any && model_shape(c.c()).din_maxw == 6);
  c = din; c.bot = {24, 65, 8};
  CHECK(model_shape(c.c()).din_any && model_shape(c.c()).din_maxw == 65);
  c = din; c.D = 6; c.bot = {18, 6, 6}; c.top = {24, 4, 1};   // D not a multiple of 4
  CHECK(model_shape(c.c()).code == DRS_OK && model_shape(c.c()).din_any);

  const Cfg dien{DRS_MODEL_DIEN, {10, 20, 30, 40, 50}, 16, {16, 8}, {56, 4, 1}, DRS_INTERACT_CAT, 0, -1, {}, 0};
  CHECK(model_shape(dien.c()).code == DRS_OK);
  c = dien; c.rows = {10, 20, 30};
  REFUSED(c, DRS_ERR_BAD_ARG, "DIEN needs at least 4 embedding tables");
  c = dien; c.bot = {16, 8, 8};
  REFUSED(c, DRS_ERR_BAD_ARG, "DIEN: ln_bot must be [D, hidden_size]");
  c = dien; c.bot = {15, 8};
  REFUSED(c, DRS_ERR_BAD_ARG, "DIEN: ln_bot must be [D, hidden_size]");
  c = dien; c.bot = {16, 0};
  REFUSED(c, DRS_ERR_BAD_ARG, "DIEN: ln_bot must be [D, hidden_size]");
  c = dien; c.top = {55, 4, 1};
  REFUSED(c, DRS_ERR_BAD_ARG, kTop);

  const Cfg ncf{DRS_MODEL_NCF, {10, 20, 30, 40}, 8, {0}, {16, 6, 4}, DRS_INTERACT_CAT, 0, -1, {}, 0};
  CHECK(model_shape(ncf.c()).code == DRS_OK && model_shape(ncf.c()).num_int == 12);
  c = ncf; c.rows = {10, 20, 30};
  REFUSED(c, DRS_ERR_BAD_ARG, "NCF has 4 embedding tables");
  c = ncf; c.top = {15, 6, 4};
  REFUSED(c, DRS_ERR_BAD_ARG, "NCF MLP branch input must be 2*D");
}

int main() {
  fixtures();
  refusals();
  printf("%d failures (%d fixture shapes)\n", fails, (int)(sizeof CASES / sizeof CASES[0]));
  return fails != 0;
}
"""


@pytest.fixture(scope="module")
def shape_main(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler builds the host program"
    d = tmp_path_factory.mktemp("model_shape")
    src = d / "shape_main.cpp"
    src.write_text(SHAPE_MAIN.replace("@CASES@", "\n".join(render(n) for n in CASES)))

    def build(name, *flags):
        exe = d / name
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-I", CSRC] + list(flags) + [str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return str(exe)
    return build


def test_the_fixtures_shapes_and_every_refusal_under_the_host_sanitizers(shape_main):
    """the header alone with -fsanitize=address,undefined, run directly: the widths derived for the seven fixture configs
    (six model kinds, DLRM with both interactions) and each refusal's code and text"""
    exe = shape_main("shape_main_san", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                     "-static-libasan", "-static-libubsan")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures (%d fixture shapes)" % len(CASES) in r.stdout, r.stdout + r.stderr


def test_the_same_program_without_the_sanitizers(shape_main):
    exe = shape_main("shape_main_o3", "-O3")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr


def test_the_fixtures_cover_the_six_kinds_and_the_lds_refusals_stay_in_drs_create():
    kinds = {case_of(n)[0]["kind"] for n in CASES}
    assert kinds == set(KIND)
    dot = case_of("dlrm_dot_small")
    assert dot[0]["op"] == "DRS_INTERACT_DOT" and case_of("dlrm_rm1_mini")[1]["num_int"] != dot[1]["num_int"]
    # what needs the kernels' word is refused where the kernels are linked, with the texts it always had
    create = open(os.path.join(CSRC, "engine_create.hip")).read()
    assert '"DIN: 4*D + 2*(widest hidden layer of a unit) floats must fit 160 KB of LDS"' in create
    assert '"DIEN: D + 4*hidden_size floats must fit 160 KB of LDS"' in create
    hdr = open(os.path.join(CSRC, "model_shape.h")).read()
    assert "hip" not in re.sub(r"//.*", "", hdr).lower()                                # plain C++: no HIP include, no HIP call
    assert "model_shape.h" in open(os.path.join(CSRC, "Makefile")).read()
