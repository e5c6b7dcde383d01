"""The rest of the reference's shouldRateLimitWorker (src/service/ratelimit.go:163-209,
customHeadersEnabled) restated as the sequential loop it is: the overall code,
the minimumDescriptor behind the RateLimit-* headers, and global shadow mode.
Helper of the verdict tests; holds no tests."""
from typing import NamedTuple, Optional

OK, OVER_LIMIT = 1, 2
MAX_U32 = 0xFFFFFFFF
FLAG_OVER_LIMIT, FLAG_GLOBAL_SHADOW = 1, 2
UNIT_SECONDS = {1: 1, 2: 60, 3: 3600, 4: 86400}


class Verdict(NamedTuple):
    code: int                  # RateLimitResponse.OverallCode
    flags: int                 # FLAG_OVER_LIMIT: finalCode before global shadow mode; FLAG_GLOBAL_SHADOW: it applied
    min_index: Optional[int]   # position of minimumDescriptor in the request, None for nil
    headers: Optional[tuple]   # (limit, remaining, reset seconds) of minimumDescriptor
    shadow_inc: int            # stats.GlobalShadowMode.Inc() calls


def verdict(statuses, is_unlimited, global_shadow) -> Verdict:
    """statuses: what DoLimit returned, objects with code, current_limit (None or
    with requests_per_unit), limit_remaining and duration_until_reset. The
    header's reset is the status's own duration_until_reset: this backend has one
    clock per request, where the reference reads its header clock just after."""
    final_code = OK                                   # :163
    min_limit_remaining = MAX_U32                     # :166
    minimum = None                                    # :167
    for i, s in enumerate(statuses):                  # :169
        if s.current_limit is not None and s.limit_remaining < min_limit_remaining:  # :171-173
            minimum = i
            min_limit_remaining = s.limit_remaining
        if is_unlimited[i]:                           # :178-182
            pass
        elif s.code == OVER_LIMIT:                    # :185-190
            final_code = s.code
            minimum = i
            min_limit_remaining = 0
    headers = None
    if minimum is not None:                           # :195-201
        m = statuses[minimum]
        headers = (m.current_limit.requests_per_unit, m.limit_remaining, m.duration_until_reset)
    flags = FLAG_OVER_LIMIT if final_code == OVER_LIMIT else 0
    inc = 0
    if final_code == OVER_LIMIT and global_shadow:    # :204-207
        final_code = OK
        flags |= FLAG_GLOBAL_SHADOW
        inc = 1
    return Verdict(final_code, flags, minimum, headers, inc)


class Status(NamedTuple):
    """A DescriptorStatus for vectors that are not built from the oracle's types."""
    code: int
    current_limit: Optional["Limit"]
    limit_remaining: int
    duration_until_reset: Optional[int]


class Limit(NamedTuple):
    requests_per_unit: int
    unit: int


def golden_statuses(case):
    """The mocked DoLimit statuses of a tests/golden/ref_service_verdict.json case;
    a limited status resets at the end of its unit's window at the case's clock
    (utils.CalculateReset)."""
    out = []
    for s in case["statuses"]:
        cl = s["current_limit"]
        if cl is None:
            out.append(Status(s["code"], None, s["limit_remaining"], None))
        else:
            div = UNIT_SECONDS[cl[1]]
            out.append(Status(s["code"], Limit(cl[0], cl[1]), s["limit_remaining"], div - case["clock"] % div))
    return out
