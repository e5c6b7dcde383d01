"""scripts/bench_scan.py on the CPU: its arguments, the prefix it measures and
the host-side filter it compares the scan with (no device: main() is not run)."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("bench_scan", os.path.join(ROOT, "scripts", "bench_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_scan_arguments():
    m = _script()
    a = m.parse_args([])
    assert (a.tenants, a.slots_log2, a.reps, a.export_reps, a.batch, a.page_records) == \
        (10_000_000, 27, 5, 2, 500_000, 1 << 20)
    a = m.parse_args(["--tenants", "1000", "--slots-log2", "12", "--reps", "2", "--export-reps", "1"])
    assert (a.tenants, a.slots_log2, a.reps, a.export_reps) == (1000, 12, 2, 1)


def test_bench_scan_prefix_selects_one_key_in_a_thousand_and_the_host_filter_agrees():
    from ratelimit_amd import abi, workloads as W
    m = _script()
    prefix, sel = m.selective_prefix(10_000_000)
    assert sel == 10_000 and len(prefix) <= abi.RL_FORGET_PREFIX_BYTES
    tenants = np.r_[np.arange(0, 30_000, 7), np.arange(9_990, 10_010), 9_999_999]
    x = W.c1_batch(tenants, W.NOW0)[0]
    L = int(x["stem_off"][1])
    stems = [r.tobytes() for r in x["stem_bytes"].reshape(-1, L)]
    hit = [s for s in stems if s.startswith(prefix)]
    assert hit == [s for s in stems if int(s[14:24]) < sel] and 0 < len(hit) < len(stems)
    assert m.selective_prefix(500) == (b"bench_tenant_t", 500)

    class FakeBackend:  # export_records(): two ranges, the second empty
        def export_records(self):
            yield {"stem_off": x["stem_off"], "stem_bytes": x["stem_bytes"], "ws": np.zeros(len(stems), np.uint32)}
            yield {"stem_off": np.zeros(1, np.uint32), "stem_bytes": np.zeros(0, np.uint8), "ws": np.zeros(0, np.uint32)}

    assert m.export_all(FakeBackend(), prefix) == (len(hit), len(stems) * L)
    assert m.export_all(FakeBackend()) == (len(stems), len(stems) * L)
    assert m.export_all(FakeBackend(), b"x" * (L + 1)) == (0, len(stems) * L)  # longer than every stem
