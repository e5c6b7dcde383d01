"""An independent pure-Python encoder and decoder of the serialized
envoy.service.ratelimit.v3.RateLimitResponse, restated from the field numbers
(go-control-plane v0.9.7) and the proto3 canonical form: fields in field-number
order, zero scalars and empty strings omitted, minimal varints, a present
sub-message written even when empty.

  RateLimitResponse: 1 overall_code, 2 statuses, 3 response_headers_to_add
  DescriptorStatus:  1 code, 2 current_limit, 3 limit_remaining, 4 duration_until_reset
  RateLimit:         1 requests_per_unit, 2 unit        Duration: 1 seconds
  HeaderValue:       1 key, 2 value

A descriptor's answer is the tuple D = (code, match, requests_per_unit, unit,
limit_remaining, reset_s) of rl_request_result's arrays; a request is a list
of them. Also holds the case lists of the response tests (the edge list and
random requests) and the sequential verdict (ratelimit.go:163-209) that turns
a request into its overall code and header values. Helper of the tests; holds
no tests and imports nothing from the product."""
import random

OK, OVER_LIMIT = 1, 2
NONE, UNLIMITED, LIMIT = 0, 1, 2
MAX_U32 = 0xFFFFFFFF
STATUS_MAX, KEY_MAX = 26, 64


def varint(v):
    assert v >= 0
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def f_varint(field, v):
    return b"" if v == 0 else varint(field << 3) + varint(v)


def f_bytes(field, data, always=True):
    return b"" if not always and not data else varint(field << 3 | 2) + varint(len(data)) + data


def encode_status(d):
    code, match, rpu, unit, rem, reset = d
    body = f_varint(1, code)
    if match == LIMIT:
        body += f_bytes(2, f_varint(1, rpu) + f_varint(2, unit))
    body += f_varint(3, rem)
    if match == LIMIT:
        body += f_bytes(4, f_varint(1, reset))
    return f_bytes(2, body)


def encode_response(code, descs, headers, keys):
    """code: the overall code; headers: (limit, remaining, reset) or None; keys: the three header names or None."""
    out = f_varint(1, code) + b"".join(encode_status(d) for d in descs)
    if keys is not None and headers is not None:
        for k, v in zip(keys, headers):
            out += f_bytes(3, f_bytes(1, bytes(k), always=False) + f_bytes(2, b"%d" % v))
    return out


def verdict_of(descs, global_shadow):
    """-> (overall code, header values or None): shouldRateLimitWorker's loop."""
    final, min_rem, minimum = OK, MAX_U32, None
    for i, (code, match, rpu, unit, rem, reset) in enumerate(descs):
        if match == LIMIT and rem < min_rem:
            minimum, min_rem = i, rem
        if match == LIMIT and code == OVER_LIMIT:
            final, minimum, min_rem = OVER_LIMIT, i, 0
    headers = None
    if minimum is not None:
        m = descs[minimum]
        headers = (m[2], m[4], m[5])
    if final == OVER_LIMIT and global_shadow:
        final = OK
    return final, headers


def encode_request(descs, global_shadow, keys):
    code, headers = verdict_of(descs, global_shadow)
    return encode_response(code, descs, headers, keys)


def bound(n_requests, n_descriptors, keys):
    per = 2 if keys is None else 2 + 3 * 16 + sum(len(k) for k in keys)
    return n_requests * per + STATUS_MAX * n_descriptors


# ---- decoder ----------------------------------------------------------------

def _fields(b):
    """[(field, wire type, value)] of one message; every field is a varint or length-delimited."""
    out, p = [], 0
    while p < len(b):
        tag, p = _rd(b, p)
        if tag & 7 == 0:
            v, p = _rd(b, p)
        else:
            assert tag & 7 == 2, tag
            n, p = _rd(b, p)
            assert p + n <= len(b)
            v, p = b[p:p + n], p + n
        out.append((tag >> 3, tag & 7, v))
    return out


def _rd(b, p):
    v = s = 0
    while True:
        c = b[p]
        p += 1
        v |= (c & 0x7F) << s
        s += 7
        if not c & 0x80:
            return v, p


def decode_response(b):
    """-> (overall code, [(code, (rpu, unit) or None, limit_remaining, reset or None)], [(key, value)])."""
    code, sts, hdrs = 0, [], []
    for f, wt, v in _fields(b):
        if f == 1 and wt == 0:
            code = v
        elif f == 2 and wt == 2:
            c, cl, rem, reset = 0, None, 0, None
            for f2, w2, v2 in _fields(v):
                if f2 == 1:
                    c = v2
                elif f2 == 2:
                    d = dict((a, x) for a, _, x in _fields(v2))
                    cl = (d.get(1, 0), d.get(2, 0))
                elif f2 == 3:
                    rem = v2
                elif f2 == 4:
                    reset = dict((a, x) for a, _, x in _fields(v2)).get(1, 0)
                else:
                    raise AssertionError(f2)
            sts.append((c, cl, rem, reset))
        elif f == 3 and wt == 2:
            d = dict((a, x) for a, _, x in _fields(v))
            hdrs.append((d.get(1, b""), d[2]))
        else:
            raise AssertionError((f, wt))
    return code, sts, hdrs


# ---- cases --------------------------------------------------------------------

U32_EDGES = [0, 1, 127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28, MAX_U32]
RESET_EDGES = [1, 59, 60, 127, 128, 3600, 16383, 16384, 86400]
KEY_SETS = [None, (b"", b"", b""), (b"L", b"R", b"T"),
            (b"RateLimit-Limit", b"RateLimit-Remaining", b"RateLimit-Reset"),
            (b"l" * 64, b"r" * 64, b"t" * 64), (b"", b"x-remaining", b"t" * 64)]
MAXIMAL = (OVER_LIMIT, LIMIT, MAX_U32, 4, MAX_U32, (1 << 21) - 1)  # a status of STATUS_MAX bytes


def edge_requests():
    """The edge list as requests: every varint width of requests_per_unit and
    limit_remaining, the reset values, each unit, the three match kinds,
    OVER_LIMIT, a request without descriptors, one without a limited
    descriptor, one of 300 descriptors."""
    reqs = []
    for i, v in enumerate(U32_EDGES):
        w = U32_EDGES[-1 - i]
        reqs.append([(OK, LIMIT, v, 1 + i % 4, w, RESET_EDGES[i % len(RESET_EDGES)])])
        reqs.append([(OK, LIMIT, v, 1 + i % 4, v, 60), (OK, LIMIT, w, 2, w, 1)])
    for r in RESET_EDGES:
        reqs.append([(OK, LIMIT, 10, 3, 5, r)])
    for u in (1, 2, 3, 4):
        reqs.append([(OK, LIMIT, 100, u, 99, 1), (OVER_LIMIT, LIMIT, 5, u, 0, 59)])
    reqs.append([(OK, NONE, 0, 0, 0, 0)])                                   # a nil limit: 12 02 08 01
    reqs.append([(OK, UNLIMITED, 0, 0, MAX_U32, 0)])                        # unlimited: 12 08 08 01 18 ff ff ff ff 0f
    reqs.append([(OK, NONE, 0, 0, 0, 0), (OK, UNLIMITED, 0, 0, MAX_U32, 0)])  # no limited descriptor: no headers
    reqs.append([])                                                         # no descriptors: 08 01
    reqs.append([(OVER_LIMIT, LIMIT, 3, 2, 0, 17), (OK, LIMIT, 9, 1, 4, 1), (OK, NONE, 0, 0, 0, 0)])
    reqs.append([(OK, LIMIT, 9, 1, 4, 1), (OVER_LIMIT, LIMIT, 3, 2, 0, 17), (OVER_LIMIT, LIMIT, 7, 4, 0, 86400)])
    reqs.append([(OK, LIMIT, 7, 1, MAX_U32, 1)])                            # a remaining of MaxUint32 is never the minimum
    reqs.append([(OK, LIMIT, 0, 1, 0, 1)])                                  # an empty RateLimit but for its unit
    reqs.append([MAXIMAL])
    reqs.append([MAXIMAL] * 5)
    reqs.append([(OK if i % 7 else OVER_LIMIT, LIMIT, 1000 + i, 1 + i % 4, 0 if i % 7 == 0 else i * 977, 1 + i % 86400)
                 for i in range(300)])
    return reqs


def random_requests(seed, n, max_desc=6):
    rng = random.Random(seed)

    def u32():
        return rng.choice([rng.choice(U32_EDGES), rng.randrange(0, 1 << rng.randrange(1, 33))])

    reqs = []
    for _ in range(n):
        descs = []
        for _ in range(rng.choice([0, 1, 1, 1, 2, 2, 3, max_desc])):
            kind = rng.choice([NONE, UNLIMITED, LIMIT, LIMIT, LIMIT])
            if kind == LIMIT:
                over = rng.random() < 0.15
                descs.append((OVER_LIMIT if over else OK, LIMIT, u32(), rng.randint(1, 4), 0 if over else u32(),
                              rng.choice([rng.choice(RESET_EDGES), rng.randint(1, 86400)])))
            else:
                descs.append((OK, kind, 0, 0, MAX_U32 if kind == UNLIMITED else 0, 0))
        reqs.append(descs)
    return reqs


def arrays_of(reqs):
    """Requests -> (req_idx, desc_first, {field: list}) in rl_request_result's names."""
    req_idx, first = [], [0]
    cols = {k: [] for k in ("code", "match", "requests_per_unit", "unit", "limit_remaining", "reset_s")}
    for q, descs in enumerate(reqs):
        for code, match, rpu, unit, rem, reset in descs:
            req_idx.append(q)
            cols["code"].append(code)
            cols["match"].append(match)
            cols["requests_per_unit"].append(rpu)
            cols["unit"].append(unit)
            cols["limit_remaining"].append(rem)
            cols["reset_s"].append(reset)
        first.append(len(req_idx))
    return req_idx, first, cols
