"""CPU-side checks of the export / import boundary (rl_export_range, rl_import):
the header declares the two entry points and the library exports them; the
ctypes mirrors of rl_records / rl_export_info equal the C compiler's layout of
include/ratelimit_hip.h field for field; Backend.import_records splits its
records into calls the ctx accepts (a stub library: no device)."""
import ctypes as C
import os
import subprocess

import numpy as np

from ratelimit_amd import abi, _lib
from ratelimit_amd.limiter import Backend, migrate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "ratelimit_hip.h")
LIB = os.path.join(ROOT, "ratelimit_amd", "libratelimit_hip.so")

MIRROR = {"rl_records": abi.RlRecords, "rl_export_info": abi.RlExportInfo}


def test_header_declares_and_library_exports_the_entry_points():
    src = open(HEADER).read()
    assert "int rl_export_range(rl_ctx* ctx, uint32_t shard, uint64_t slot_begin, uint64_t slot_end" in src
    assert "int rl_import(rl_ctx* ctx, const rl_records* in);" in src
    assert "rl_export_range" in _lib.EXPORTS and "rl_import" in _lib.EXPORTS
    if not os.path.exists(LIB):
        from ratelimit_amd import build
        build.build()
    lib = C.CDLL(LIB)
    assert hasattr(lib, "rl_export_range") and hasattr(lib, "rl_import")
    lib.rl_abi_version.restype = C.c_uint32
    assert lib.rl_abi_version() == abi.ABI_VERSION >= 7


def _layout_program():
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "ratelimit_hip.h"',
             '#define F(s, f) printf("F %s %s %u %u\\n", #s, #f, (unsigned)offsetof(s, f), '
             '(unsigned)sizeof(((s*)0)->f))',
             'int main(void) {']
    for name, cls in MIRROR.items():
        lines.append('  printf("S %s %%u\\n", (unsigned)sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            lines.append("  F(%s, %s);" % (name, f))
    lines += ['  printf("C RL_REC_CHAIN_LOST %u\\n", (unsigned)RL_REC_CHAIN_LOST);', "  return 0;", "}"]
    return "\n".join(lines) + "\n"


def test_records_structs_match_the_c_layout(tmp_path):
    src = tmp_path / "migrate_layout.c"
    src.write_text(_layout_program())
    exe = str(tmp_path / "migrate_layout")
    subprocess.run(["gcc", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + INC, str(src),
                    "-o", exe], check=True, capture_output=True, text=True)
    sizes, fields, consts = {}, {}, {}
    for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n"):
        p = ln.split()
        if not p:
            continue
        if p[0] == "S":
            sizes[p[1]] = int(p[2])
        elif p[0] == "F":
            fields.setdefault(p[1], []).append((p[2], int(p[3]), int(p[4])))
        else:
            consts[p[1]] = int(p[2])
    assert set(sizes) == set(MIRROR)
    for name, cls in MIRROR.items():
        assert C.sizeof(cls) == sizes[name], name
        mirror = [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_]
        assert mirror == fields[name], name  # the same fields in the same order, offsets and sizes
    assert consts == {"RL_REC_CHAIN_LOST": abi.RL_REC_CHAIN_LOST}
    assert C.sizeof(abi.RlRecords) == 16 + 8 * 8 and C.sizeof(abi.RlExportInfo) == 6 * 8


class StubLib:
    """Stands for the library: records what rl_import was given."""

    def __init__(self, fail_at=None):
        self.calls = []
        self.fail_at = fail_at

    def rl_import(self, ctx, ref):
        r = ref._obj
        n = r.n

        def arr(p, dt, m):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(dt)), (m,)).copy() if m else np.zeros(0, dt)

        off = arr(r.stem_off, C.c_uint32, n + 1)
        call = {"stem_off": off, "stem_bytes": arr(r.stem_bytes, C.c_uint8, int(off[n]))}
        for k, dt in (("unit", C.c_uint8), ("flags", C.c_uint8), ("ws", C.c_uint32), ("count", C.c_uint32),
                      ("expire", C.c_uint32), ("lc", C.c_uint32)):
            call[k] = arr(getattr(r, k), dt, n)
        self.calls.append(call)
        return abi.RL_E_TABLE_FULL if self.fail_at == len(self.calls) else abi.RL_OK

    def rl_last_error(self, ctx):
        return b"gpu: counter table full (stub)"


def _stub_backend(max_batch, max_stem_bytes=0, **kw):
    be = Backend.__new__(Backend)
    be.L = StubLib(**kw)
    be.ctx = None  # (close() then has nothing to destroy)
    be.cfg = abi.RlConfig()
    be.cfg.max_batch, be.cfg.max_stem_bytes, be.cfg.n_shards = max_batch, max_stem_bytes, 1
    return be


def _records(n, seed=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 70, n)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    return {"stem_bytes": rng.integers(32, 127, int(off[n])).astype(np.uint8), "stem_off": off,
            "unit": rng.integers(1, 5, n).astype(np.uint8), "flags": rng.integers(0, 2, n).astype(np.uint8),
            "ws": (rng.integers(0, 1000, n) * 86400).astype(np.uint32), "count": rng.integers(0, 99, n).astype(np.uint32),
            "expire": rng.integers(0, 1 << 31, n).astype(np.uint32), "lc": rng.integers(0, 1 << 31, n).astype(np.uint32)}


def _joined(calls):
    out = {k: np.concatenate([c[k] for c in calls]) for k in calls[0] if k != "stem_off"}
    lens = np.concatenate([np.diff(c["stem_off"].astype(np.int64)) for c in calls])
    out["stem_off"] = np.r_[0, np.cumsum(lens)].astype(np.uint32)
    return out


def test_import_records_splits_at_max_batch():
    rec = _records(2500)
    be = _stub_backend(1000)
    assert be.import_records(rec) == 3
    calls = be.L.calls
    assert [len(c["ws"]) for c in calls] == [1000, 1000, 500]
    for c in calls:  # every call is a batch of its own: offsets rebased, stems cut to match
        assert c["stem_off"][0] == 0 and len(c["stem_bytes"]) == c["stem_off"][-1]
    j = _joined(calls)
    for k, v in rec.items():
        assert np.array_equal(j[k], v), k
    # an exact multiple, a single call and an empty set
    be = _stub_backend(500)
    assert be.import_records(_records(1000, 1)) == 2 and [len(c["ws"]) for c in be.L.calls] == [500, 500]
    be = _stub_backend(0)  # (0: the library's default, 1 << 20)
    assert be.import_records(rec) == 1 and len(be.L.calls[0]["ws"]) == 2500
    empty = {k: v[:0] if k != "stem_off" else v[:1] for k, v in rec.items()}
    assert _stub_backend(10).import_records(empty) == 0


def test_import_records_splits_at_max_stem_bytes():
    rec = _records(400, 2)
    be = _stub_backend(1000, max_stem_bytes=1024)
    n_calls = be.import_records(rec)
    assert n_calls == len(be.L.calls) > 1
    assert all(c["stem_off"][-1] <= 1024 for c in be.L.calls)
    j = _joined(be.L.calls)
    for k, v in rec.items():
        assert np.array_equal(j[k], v), k


def test_import_records_raises_the_library_status():
    import pytest
    from ratelimit_amd.limiter import RedisError
    be = _stub_backend(100, fail_at=2)
    with pytest.raises(RedisError, match="RL_E_TABLE_FULL") as e:
        be.import_records(_records(250, 3))
    assert e.value.status == abi.RL_E_TABLE_FULL and len(be.L.calls) == 2  # stops at the failed call


def test_migrate_is_exported():
    import ratelimit_amd.limiter as Lm
    assert "migrate" in Lm.__all__ and callable(migrate)
