"""scripts/bench_forget.py on the CPU: its arguments and the prefix sets it
measures (no device: main() is not run)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("bench_forget", os.path.join(ROOT, "scripts", "bench_forget.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bench_forget_arguments():
    m = _script()
    a = m.parse_args([])
    assert (a.tenants, a.slots_log2, a.keys, a.reps, a.batch) == (10_000_000, 27, 1 << 20, 5, 500_000)
    a = m.parse_args(["--tenants", "1000", "--slots-log2", "12", "--keys", "64", "--reps", "2"])
    assert (a.tenants, a.slots_log2, a.keys, a.reps) == (1000, 12, 64, 2)


def test_bench_forget_prefix_sets_select_what_they_say():
    from ratelimit_amd import abi, workloads as W
    import numpy as np
    m = _script()
    tenants = 250_000
    x = W.c1_batch(np.arange(tenants), W.NOW0)[0]
    L = int(x["stem_off"][1])
    stems = [r.tobytes() for r in x["stem_bytes"].reshape(-1, L)[::97]]  # (a sample: every 97th key)
    for case, (prefixes, sel) in m.prefix_sets(tenants).items():
        assert len(prefixes) == int(case.split("_")[0]) <= abi.RL_FORGET_PREFIX_MAX, case
        assert sum(map(len, prefixes)) <= abi.RL_FORGET_PREFIX_BYTES and all(prefixes)
        hit = [s for s in stems if any(s.startswith(p) for p in prefixes)]
        if not sel:
            assert not hit, case
        else:
            assert sel == 100_000 and hit == [s for s in stems if int(s[14:24]) < sel], case
    assert all(p[:4] != stems[0][:4] for p in m.prefix_sets(tenants)["64_selective"][0])
    assert all(p[:14] == stems[0][:14] for p in m.prefix_sets(tenants)["64_selective_shared_head"][0])
