"""The greedy per-table pass of DLRM_Net.tune_table_placement ("sls_nt_mask") against a scripted gather time (no GPU).

The stub's "gather us" is a fixed function of the mask plus bounded noise: every table has a policy it is faster under,
worth `gain[t]` us.  The pass must find the per-table optimum when the flips are worth more than the spread of a reading,
keep the uniform mask when they are worth less, and never read more than (T + 1) * K times.
"""
import numpy as np

from deeprecsys_amd import dlrm_s_hip as M

T, K = 8, 3


def stub(best, gain, noise, seed=0):
    rng = np.random.RandomState(seed)
    calls = []

    def read(mask):
        calls.append(mask)
        wrong = [t for t in range(T) if ((mask >> t) & 1) != ((best >> t) & 1)]
        return 80.0 + sum(gain[t] for t in wrong) + rng.uniform(-noise, noise)
    return read, calls


def test_the_pass_finds_the_per_table_optimum_when_flips_beat_the_spread():
    for best in (0b00000011, 0b10110100, 0b11111111, 0):
        for start in (0, (1 << T) - 1):
            read, calls = stub(best, [0.6] * T, noise=0.05, seed=best + start)
            mask, us, spread, flips, start_us = M.DLRM_Net.greedy_nt_mask(read, T, start, k=K)
            assert mask == best and len(calls) == (T + 1) * K and len(flips) == T
            assert spread <= 0.1 and abs(us - 80.0) <= 0.05 and us <= start_us


def test_the_pass_keeps_the_uniform_mask_when_flips_are_inside_the_spread():
    # the starting mask reads 80.0 / 80.5 / 80.25 (median 80.25, spread 0.5); every flip reads 80.0 +- 0.05: 0.25 us better,
    # inside the spread -- nothing is kept, and the record says what the flips read
    start_reads = [80.0, 80.5, 80.25]
    rng = np.random.RandomState(1)
    calls = []

    def read(mask):
        calls.append(mask)
        return start_reads[len(calls) - 1] if len(calls) <= K else 80.0 + rng.uniform(-0.05, 0.05)
    full = (1 << T) - 1
    mask, us, spread, flips, start_us = M.DLRM_Net.greedy_nt_mask(read, T, full, k=K)
    assert mask == full and us == 80.25 == start_us and spread == 0.5 and len(calls) == (T + 1) * K
    assert all(abs(u - 80.0) <= 0.05 for u in flips)
    assert calls[:K] == [full] * K and calls[K:2 * K] == [full ^ 1] * K


def test_a_flip_must_beat_the_median_by_more_than_the_spread():
    # exact readings: spread 0 -- every helpful flip is kept, an unhelpful one never
    read, calls = stub(0b00001111, [1.0] * T, noise=0.0)
    mask, us, spread, flips, start_us = M.DLRM_Net.greedy_nt_mask(read, T, 0, k=K)
    assert mask == 0b00001111 and spread == 0.0 and us == 80.0 and start_us == 84.0
    assert flips == [83.0, 82.0, 81.0, 80.0, 81.0, 81.0, 81.0, 81.0]


def test_tune_table_placement_keeps_the_found_uniform_policy_when_every_bit_flips():
    """The whole search on a scripted engine: a mixed mask is set and recorded; a pass that flips every table ends on the
    other uniform policy, which is then the engine's "sls_nt" with the mask unset."""

    class Eng:
        max_batch, num_slots = 256, 3

        def __init__(self, best):
            self.best = best
            self.opt = {"gather_bound": 1, "preferred_coalesce": 12, "preferred_slots": 3, "sls_nt": 1, "sls_nt_mask": -1,
                        "table_bytes": 2 << 30, "table_alloc": 0, "table_dtype": 0, "dispatch_log": 0}
            self.user_options, self.reads = set(), 0

        def get_option(self, k): return self.opt[k]

        def set_option(self, k, v, user=True):
            if k == "table_placement" and v == -1:
                raise M.N.DrsError(-2, "drs_set_option", "no room")
            self.opt[k] = v

        def forward_multi_async(self, *a): pass
        def wait(self, *a): pass
        def reset_kernel_time(self): pass
        def set_profiling(self, *a): pass
        def last_dispatch(self, slot=0): return ["sls_flatc_ntm_kernel<16,20,ntm=0x1>[5 wg, L=80]"] if self.opt["sls_nt_mask"] > 0 else []

        def kernel_time(self, _k):
            self.reads += 1
            m = self.opt["sls_nt_mask"]
            m = m if m >= 0 else (0b111 if self.opt["sls_nt"] else 0)
            return (80.0 + bin(m ^ self.best).count("1")) * 1e-3, 1

    def run(best):
        net = M.DLRM_Net.__new__(M.DLRM_Net)
        net.engine, net._n_staged, net.ln_emb = Eng(best), 4, np.array([10, 10, 10])
        return net.tune_table_placement(2, sets=4), net.engine

    rec, eng = run(0b101)
    assert rec["sls_nt_mask"] == "0x5" and eng.opt["sls_nt_mask"] == 0b101 and rec["mask_readings"] == 12 and len(rec["mask_flip_us"]) == 3
    rec, eng = run(0b000)       # all-ones start (nt reads 83, plain 80: plain is kept by the arena search, nothing to flip)
    assert rec["sls_nt_mask"] is None and eng.opt["sls_nt_mask"] == -1 and eng.opt["sls_nt"] == 0
