"""The Go adapter (go/src/gpu, go/src/config, go/patches) against the C ABI.

There is no Go toolchain here, so the Go side is checked from
its text, against what a compiler would check at the cgo boundary:

* every cgo preamble compiles as C against include/ratelimit_hip.h;
* every C.<name> the Go files use exists in the header: functions with the
  arity of each call, RL_* constants, rl_* types, and every C struct field
  the Go code reads or writes (offsetof, compiled);
* the runner patch calls the constructor with createLimiter's own arguments
  (src/service_cmd/runner/runner.go:50) and every settings field the adapter
  reads is one the settings patch adds or the reference already has;
* INTEGRATION.md holds no Go code of its own (it points at these files).
"""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GO = os.path.join(ROOT, "go")
HEADER = os.path.join(ROOT, "include", "ratelimit_hip.h")
CGO_BUILTINS = {"GoString", "GoStringN", "GoBytes", "CString", "CBytes"}
C_SCALARS = {"uint8_t", "uint16_t", "uint32_t", "uint64_t", "int8_t", "int16_t", "int32_t", "int64_t", "float",
             "double", "char", "int", "uint", "size_t", "uchar", "schar", "short", "ushort", "long", "ulong"}
LIBC = {"malloc", "calloc", "free", "memset", "memcpy"}


def go_files(sub="src"):
    out = []
    for d, _, fs in os.walk(os.path.join(GO, sub)):
        out += [os.path.join(d, f) for f in sorted(fs) if f.endswith(".go")]
    return out


def strip_go(src):
    """Go source without comments and string literals (cgo preambles removed too)."""
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r'"(?:\\.|[^"\\])*"', '""', src)
    src = re.sub(r"`[^`]*`", '""', src)
    return src


def header_api():
    h = open(HEADER).read()
    hs = re.sub(r"/\*.*?\*/", " ", h, flags=re.S)
    funcs = {}
    for m in re.finditer(r"\b(rl_\w+)\s*\(([^;{]*?)\)\s*;", hs, flags=re.S):
        args = m.group(2).strip()
        funcs[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    consts = set(re.findall(r"#define\s+(RL_\w+)", hs)) | set(re.findall(r"\b(RL_\w+)\s*=", hs))
    types = set(re.findall(r"}\s*(rl_\w+)\s*;", hs)) | set(re.findall(r"typedef\s+struct\s+\w+\s+(rl_\w+)\s*;", hs))
    return funcs, consts, types


def call_args(src, start):
    """Number of top-level arguments of the call whose '(' is at src[start]."""
    depth, n, empty = 0, 1, True
    for i in range(start, len(src)):
        ch = src[i]
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                return 0 if empty else n
        elif ch == "," and depth == 1:
            n += 1
        elif depth >= 1 and not ch.isspace():
            empty = False
    raise AssertionError("unbalanced call")


def gcc_syntax(code, tag):
    with tempfile.NamedTemporaryFile("w", suffix=".c", delete=False, prefix=tag) as f:
        f.write(code)
        path = f.name
    try:
        r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.dirname(HEADER),
                            path], capture_output=True, text=True)
        assert r.returncode == 0, "%s:\n%s\n%s" % (tag, r.stderr, code)
    finally:
        os.unlink(path)


def test_go_adapter_files_exist():
    names = {os.path.relpath(p, GO) for p in go_files()}
    for f in ("src/gpu/gpu.go", "src/gpu/cache_impl.go", "src/gpu/stats.go", "src/gpu/config.go",
              "src/gpu/comm.go", "src/gpu/requests.go", "src/config/walk.go", "src/limiter/request_cache.go"):
        assert f in names, f
    for p in ("settings.go.patch", "runner.go.patch", "Dockerfile.patch", "ratelimit.go.patch"):
        assert os.path.exists(os.path.join(GO, "patches", p)), p


@pytest.mark.parametrize("path", [p for p in go_files() if 'import "C"' in open(p).read()],
                         ids=lambda p: os.path.relpath(p, GO))
def test_cgo_preamble_compiles_against_header(path):
    src = open(path).read()
    m = re.search(r"/\*(.*?)\*/\s*import \"C\"", src, flags=re.S)
    assert m, "no cgo preamble before import \"C\""
    pre = "\n".join(l for l in m.group(1).splitlines() if not l.strip().startswith("#cgo"))
    assert '#include "ratelimit_hip.h"' in pre
    gcc_syntax(pre + "\nint main(void) { return (int)rl_abi_version() * 0; }\n", "preamble_")


def test_go_c_references_exist_in_header():
    funcs, consts, types = header_api()
    fields = set()  # (C type, field)
    checked_calls = 0
    for path in go_files():
        raw = open(path).read()
        if 'import "C"' not in raw:
            continue
        src = strip_go(raw)
        # variables / fields / params of C struct types, and slices of them
        typed = {}
        for m in re.finditer(r"\bvar\s+(\w+)\s+C\.(rl_\w+)", src):
            typed[m.group(1)] = m.group(2)
        for m in re.finditer(r"^\s*(\w+)\s+\*?C\.(rl_\w+)\s*$", src, flags=re.M):
            typed[m.group(1)] = m.group(2)
        for m in re.finditer(r"[(,]\s*(\w+)\s+\*C\.(rl_\w+)", src):
            typed[m.group(1)] = m.group(2)
        elem = {}
        for m in re.finditer(r"\b(\w+)\s+\[\]C\.(rl_\w+)", src):
            elem[m.group(1)] = m.group(2)
        for m in re.finditer(r"\b(\w+)\s*:=\s*\(\*\[[^\]]+\]C\.(rl_\w+)\)", src):
            elem[m.group(1)] = m.group(2)
        for m in re.finditer(r"\b(\w+)\s*:=\s*&(?:\w+\.)*(\w+)\[", src):
            if m.group(2) in elem:
                typed[m.group(1)] = elem[m.group(2)]
        for m in re.finditer(r"C\.(rl_\w+)\{(\w+)\s*:", src):
            fields.add((m.group(1), m.group(2)))
        for name, t in typed.items():
            if t in ("rl_ctx", "rl_packer"):  # opaque handles: no fields (a Go field of that type is not one)
                continue
            for m in re.finditer(r"(?<![\w])%s\.([a-z_][a-z0-9_]*)\b" % re.escape(name), src):
                fields.add((t, m.group(1)))
        for m in re.finditer(r"\bC\.(\w+)", src):
            name = m.group(1)
            after = src[m.end():m.end() + 1]
            if name in CGO_BUILTINS or name in C_SCALARS or name in LIBC:
                continue
            if name.startswith("RL_"):
                assert name in consts, "%s: C.%s is not in the header" % (os.path.basename(path), name)
            elif name in types:
                continue
            elif name in funcs:
                assert after == "(", name
                n = call_args(src, m.end())
                assert n == funcs[name], "%s: C.%s called with %d arguments, header has %d" % (
                    os.path.basename(path), name, n, funcs[name])
                checked_calls += 1
            else:
                raise AssertionError("%s: C.%s is not declared by the header" % (os.path.basename(path), name))
    assert checked_calls >= 15, checked_calls
    assert len(fields) >= 40, sorted(fields)
    code = ['#include <stddef.h>', '#include "ratelimit_hip.h"', "int main(void) {", "  size_t s = 0;"]
    code += ["  s += offsetof(%s, %s);" % tf for tf in sorted(fields)]
    code += ["  return (int)s * 0;", "}"]
    gcc_syntax("\n".join(code) + "\n", "fields_")


def _added(patch):
    return "\n".join(l[1:] for l in open(os.path.join(GO, "patches", patch)).read().splitlines()
                     if l.startswith("+") and not l.startswith("+++"))


def test_runner_and_settings_patches_match_the_adapter():
    impl = strip_go(open(os.path.join(GO, "src", "gpu", "cache_impl.go")).read())
    m = re.search(r"func NewRateLimitCacheImplFromSettings\(([^)]*)\)\s*limiter\.RateLimitCache", impl)
    assert m, "constructor missing"
    params = [p.strip().split()[-1] for p in m.group(1).split(",")]
    assert params == ["settings.Settings", "*freecache.Cache", "server.Server", "utils.TimeSource", "stats.Manager"]
    # createLimiter(srv server.Server, s settings.Settings, localCache *freecache.Cache, statsManager stats.Manager)
    # (runner.go:50): the case passes its own parameters, in the constructor's order
    run = _added("runner.go.patch")
    c = re.search(r'case "gpu":\s*return gpu\.NewRateLimitCacheImplFromSettings\((.*?)\)\s*$', run, flags=re.S | re.M)
    assert c, run
    args = [a.strip() for a in c.group(1).split(",") if a.strip()]
    assert args == ["s", "localCache", "srv", "utils.NewTimeSourceImpl()", "statsManager"], args
    assert '"github.com/envoyproxy/ratelimit/src/gpu"' in run
    # every s.X the adapter reads: added by the settings patch, or a reference setting
    added = set(re.findall(r"^\s*(\w+)\s+\S+\s+`envconfig", _added("settings.go.patch"), flags=re.M))
    reference = {"NearLimitRatio", "RedisPerSecond", "ExpirationJitterMaxSeconds", "CacheKeyPrefix",
                 "LocalCacheSizeInBytes"}
    body = impl[m.start():impl.index("\nfunc ", m.end())]
    used = set(re.findall(r"\bs\.(\w+)", body))
    assert used and used <= added | reference, used - added - reference
    assert {u for u in used if u.startswith("Gpu")} <= added
    assert "CGO_ENABLED=1" in _added("Dockerfile.patch")


def test_dockerfile_build_and_final_stages_share_the_rocm_base():
    """The build stage links libratelimit_hip.so, whose DT_NEEDED entries
    (libamdhip64, glibc 2.35) must resolve at link time: it runs on the same
    ROCm base image as the final stage, with Go installed, and passes
    -rpath-link for the ROCm libraries (round-4 review, missing #2)."""
    dk = _added("Dockerfile.patch")
    froms = re.findall(r"^FROM\s+(\S+)(?:\s+AS\s+(\w+))?", dk, flags=re.M)
    stages = {alias: image for image, alias in froms}
    assert stages.get("build") == "base" and stages.get("final") == "base", froms
    assert stages.get("base", "").startswith("rocm/"), froms
    assert not any(img.startswith(("golang", "alpine")) for img, _ in froms), froms
    assert "go${GO_VERSION}.linux-amd64.tar.gz" in dk
    assert re.search(r"CGO_LDFLAGS=\"[^\"]*-rpath-link,/opt/rocm/lib", dk)
    # the binary finds the library where the cgo rpath points (gpu.go: ${SRCDIR}/../../third_party/...)
    gpu = open(os.path.join(GO, "src", "gpu", "gpu.go")).read()
    assert "-Wl,-rpath,${SRCDIR}/../../third_party/ratelimit_hip/lib" in gpu
    assert "WORKDIR /ratelimit" in open(os.path.join(GO, "patches", "Dockerfile.patch")).read()
    assert "/ratelimit/third_party/ratelimit_hip/lib/" in dk


def _hunks(patch):
    """(target, [(old start, old lines)]) of a one-file unified diff: each
    hunk's context and removed lines, i.e. what `patch` must find in the file."""
    lines = open(os.path.join(GO, "patches", patch)).read().split("\n")
    target = re.match(r"--- a/(\S+)", lines[0]).group(1)
    assert re.match(r"\+\+\+ b/%s\b" % re.escape(target), lines[1]), lines[1]
    hunks, i = [], 2
    while i < len(lines) and lines[i].startswith("@@"):
        m = re.match(r"@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@", lines[i])
        assert m, lines[i]
        n_old, n_new = int(m.group(2) or 1), int(m.group(4) or 1)
        old, new, i = [], 0, i + 1
        while len(old) < n_old or new < n_new:
            tag, text = lines[i][:1], lines[i][1:]
            assert tag in (" ", "-", "+", "\\"), (patch, i, lines[i])
            if tag in (" ", "-"):
                old.append(text)
            if tag in (" ", "+"):
                new += 1
            i += 1
        assert len(old) == n_old and new == n_new, (patch, m.group(0))
        hunks.append((int(m.group(1)), old))
    assert hunks and all(not l for l in lines[i:]), (patch, lines[i:i + 3])
    return target, hunks


def test_patches_apply_to_the_reference():
    """Every hunk of go/patches/*.patch finds all its context and removed
    lines, unchanged and in order, in the reference file it patches (no fuzz;
    stricter than `patch --dry-run`). The reference files stand in as per-line
    digests (tests/golden/ref_patch_targets.json, make_golden_patch_targets.py)."""
    import hashlib
    import json
    with open(os.path.join(ROOT, "tests", "golden", "ref_patch_targets.json")) as f:
        files = json.load(f)["files"]
    seen = set()
    for p in ("settings.go.patch", "runner.go.patch", "Dockerfile.patch", "ratelimit.go.patch"):
        target, hunks = _hunks(p)
        ref = files[target]
        seen.add(target)
        at = 0  # hunks apply top to bottom, none over the one before
        for start, old in hunks:
            want = [hashlib.sha256(l.encode()).hexdigest()[:16] for l in old]
            found = [k for k in range(at, len(ref) - len(want) + 1) if ref[k:k + len(want)] == want]
            assert found, "%s: the hunk at line %d does not apply to %s" % (p, start, target)
            # at its stated line, or (as `patch` does) the nearest place where it applies
            k = min(found, key=lambda k: abs(k - (start - 1)))
            at = k + len(want)
    assert seen == set(files), seen ^ set(files)


def test_integration_md_points_at_the_go_files():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "```go" not in text, "Go code belongs in go/src, not in INTEGRATION.md"
    for f in ("go/src/gpu/gpu.go", "go/src/gpu/cache_impl.go", "go/patches/runner.go.patch"):
        assert f in text, f


def test_config_match_reaches_the_service():
    """GPU_CONFIG_MATCH (round-4 review, missing #4): the service patch hands
    every loaded config to a limiter.RequestRateLimitCache and asks it first
    for the whole request; the GPU cache implements both methods with the
    interface's signatures, loads the config with Ctx.LoadConfig from its
    batcher and answers raw requests through rl_do_limit_requests."""
    iface = strip_go(open(os.path.join(GO, "src", "limiter", "request_cache.go")).read())
    assert re.search(r"ConfigLoaded\(cfg config\.RateLimitConfig\)", iface)
    assert re.search(r"DoLimitRequest\(ctx context\.Context, request \*pb\.RateLimitRequest\)", iface)
    svc = _added("ratelimit.go.patch")
    assert "this.cache.(limiter.RequestRateLimitCache)" in svc
    assert "rc.ConfigLoaded(newConfig)" in svc and "rc.DoLimitRequest(ctx, request)" in svc
    # the fallback keeps the reference path: GetLimit in Go, then DoLimit
    assert "this.constructLimitsToCheck(request, ctx)" in svc and "this.cache.DoLimit(ctx, request, limitsToCheck)" in svc
    impl = strip_go(open(os.path.join(GO, "src", "gpu", "cache_impl.go")).read())
    assert re.search(r"func \(this \*rateLimitCacheImpl\) ConfigLoaded\(cfg config\.RateLimitConfig\)", impl)
    assert re.search(r"func \(this \*rateLimitCacheImpl\) DoLimitRequest\(ctx context\.Context, "
                     r"request \*pb\.RateLimitRequest\)", impl)
    assert "this.ctx.LoadConfig(cfg, this.prefix, this.rule)" in impl
    assert "this.ctx.DoLimitRequests(b)" in impl
    assert "s.GpuConfigMatch" in impl
    assert re.search(r"GpuConfigMatch\s+bool\s+`envconfig:\"GPU_CONFIG_MATCH\"", _added("settings.go.patch"))
    # override stats keys as the reference names them (config_impl.go:300-312)
    assert 'return domain + "." + strings.Join(parts, ".")' in open(os.path.join(GO, "src", "gpu", "cache_impl.go")).read()


def test_routed_ctx_has_a_go_entry_point():
    """One process per GPU (round-4 review, weak #7): no exported Go API takes
    cgo types; a routed ctx takes the batcher's prefix-shared batches (Submit)
    and the batcher of a routed ctx submits one collective batch per tick."""
    for path in go_files():
        src = strip_go(open(path).read())
        for m in re.finditer(r"^func (?:\([^)]*\) )?([A-Z]\w*)\(([^)]*)\)", src, flags=re.M):
            assert "C." not in m.group(2), (os.path.basename(path), m.group(1), m.group(2))
    comm = strip_go(open(os.path.join(GO, "src", "gpu", "comm.go")).read())
    assert "RoutedDoLimit" not in comm and "func CommIDFile(" in comm and "func (c *Ctx) CommInit(" in comm
    impl = strip_go(open(os.path.join(GO, "src", "gpu", "cache_impl.go")).read())
    assert "go this.batcherRouted()" in impl and "ctx.CommInit(s.GpuWorld, s.GpuRank, id)" in impl


def test_go_struct_literals_are_keyed():
    """No positional literal of a multi-field struct declared in go/src, and
    every key a declared field (tests/go_lint.py: the composite-literal part
    of `go vet`, which this image cannot run)."""
    import go_lint
    findings, types = go_lint.lint_tree(os.path.join(GO, "src"))
    assert not findings, "\n".join(findings)
    assert {"call", "flight", "reply", "TableInfo", "Options"} <= set(types["gpu"])


def test_go_lint_names_the_round5_call_literal():
    """Round 5's `&call{request, limits, now, done}` (4 values; `call` has 6
    fields) is flagged; its keyed form is not; an unknown key is."""
    import go_lint
    src = open(os.path.join(GO, "src", "gpu", "cache_impl.go")).read()
    types = go_lint.struct_fields(src)
    assert len(types["call"]) == 6, types["call"]
    bad = "func f() { c := &call{request, limits, this.timeSource.UnixNow(), make(chan reply, 1)} }"
    f = go_lint.lint_source(bad, types, path="cache_impl.go")
    assert any("positional literal of a 6-field struct (4 values)" in x for x in f), f
    good = "func f() { c := &call{req: request, limits: limits, now: 1, done: make(chan reply, 1)} }"
    assert go_lint.lint_source(good, types) == []
    assert go_lint.lint_source("func f() { _ = reply{error: \"x\"} }", types)  # (the field is err)
    # slice literals of the type and the type's own declaration are not struct literals
    assert go_lint.lint_source("func f() { calls := []*call{first}; _ = calls }", types) == []


def test_device_failures_flip_the_health_check():
    """GPU loss fails the server's health check (the Redis pool does
    it on its connections, src/redis/driver_impl.go:31-52): the batcher feeds
    every batch's, request batch's and sweep's outcome to healthMonitor, which
    calls srv.HealthCheckFail() on a device-level rl_status and HealthCheckOK()
    at the next success; GPU_HEALTH_CHECK_DEVICE (default true) enables it."""
    impl = strip_go(open(os.path.join(GO, "src", "gpu", "cache_impl.go")).read())
    for fn in ("finish", "doRaw", "housekeeping"):
        m = re.search(r"func \(this \*rateLimitCacheImpl\) %s\(" % fn, impl)
        nxt = impl.find("\nfunc ", m.end())
        body = impl[m.end():nxt if nxt >= 0 else len(impl)]
        assert "this.health.observe(" in body, fn
    m = re.search(r"func \(h \*healthMonitor\) observe\(err error\) \{", impl)
    body = impl[m.end():impl.index("\nfunc ", m.end()) if "\nfunc " in impl[m.end():] else len(impl)]
    assert "h.srv.HealthCheckFail()" in body and "h.srv.HealthCheckOK()" in body
    dev = re.search(r"func deviceFailure\(err error\) bool \{(.*?)\n\}", impl, flags=re.S).group(1)
    assert "StatusHIP" in dev and "StatusComm" in dev and "StatusInternal" in dev
    gpu = strip_go(open(os.path.join(GO, "src", "gpu", "gpu.go")).read())
    for name, c in (("StatusHIP", "RL_E_HIP"), ("StatusComm", "RL_E_COMM"), ("StatusInternal", "RL_E_INTERNAL")):
        assert re.search(r"%s\s*=\s*int\(C\.%s\)" % (name, c), gpu), name
    ctor = impl[impl.index("func NewRateLimitCacheImplFromSettings("):]
    assert "s.GpuHealthCheckDevice && srv != nil" in ctor and "opt.HealthServer = srv" in ctor
    assert re.search(r"GpuHealthCheckDevice\s+bool\s+`envconfig:\"GPU_HEALTH_CHECK_DEVICE\" default:\"true\"`",
                     _added("settings.go.patch"))


def test_local_cache_gauges_are_the_reference_eight():
    """limiter.localCacheStats publishes eight freecache gauges
    (src/limiter/local_cache_stats.go:20-43) and the reference's gauge test
    checks that every one exists (fixed_cache_impl_test.go:150-167): the GPU
    adapter registers the same names."""
    names = {"evacuateCount", "expiredCount", "entryCount", "averageAccessTime", "hitCount", "missCount",
             "lookupCount", "overwriteCount"}
    src = open(os.path.join(GO, "src", "gpu", "stats.go")).read()
    got = set(re.findall(r'scope\.NewGauge\("(\w+)"\)', src))
    assert got == names, got ^ names
    gen = src[src.index("func (s localCacheStats) GenerateStats()"):]
    assert all(("s.%s.Set(" % n) in gen for n in names)
