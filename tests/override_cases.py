"""Serialized RateLimitRequest messages whose descriptors carry a ``limit``
override, for the device interner's tests (the CPU driver in
test_wire_override_cpu.py, the kernels in test_gpu_wire_override.py), and what
the host packer, the authority, says about one message's overrides."""
import numpy as np

from ratelimit_amd._lib import RedisError
from ratelimit_amd.config import batch_arrays
import pbwire
import wire_cases as WC

fb, fv = pbwire.field_bytes, pbwire.field_varint


def entry(k=b"k", v=b"v"):
    return fb(1, (fb(1, k) if k else b"") + (fb(2, v) if v else b""))


def limit(rpu=None, unit=None):
    return fb(2, (fv(1, rpu) if rpu is not None else b"") + (fv(2, unit) if unit is not None else b""))


def desc(*parts):
    """A RateLimitDescriptor of the given entries and limit fields, in that order."""
    return fb(2, b"".join(parts))


def message(domain, *descs, hits=None):
    return (fb(1, domain) if domain is not None else b"") + b"".join(descs) + (fv(3, hits) if hits is not None else b"")


def named_cases():
    """-> [(name, message)]: the shapes the override walk must parse as the packer does."""
    dom = fb(1, b"domain_1")
    d_plain = desc(entry(b"key_x", b"a_b"))
    d_ov = desc(entry(b"key_x", b"a_b"), limit(10, 1))
    return [
        ("domain_after_descriptors", d_ov + d_plain + dom),
        ("domain_twice_around", fb(1, b"first") + d_ov + dom),
        ("no_domain", d_ov),
        ("two_limits_last_wins", dom + desc(entry(), limit(10, 1), limit(7, 3))),
        ("two_limits_merge_fields", dom + desc(limit(10, None), entry(), limit(None, 2))),
        ("limit_fields_repeated", dom + desc(entry(), fb(2, fv(1, 3) + fv(2, 4) + fv(1, 9) + fv(2, 2)))),
        ("limit_before_entries", dom + desc(limit(5, 2), entry(b"a", b"b"), entry(b"c", b"d"))),
        ("empty_limit", dom + desc(entry(), fb(2, b""))),
        ("limit_unknown_fields", dom + desc(entry(), fb(2, fv(9, 1) + fv(1, 4) + fb(7, b"xyz") + fv(2, 1)))),
        ("limit_wrong_wire_types", dom + desc(entry(), fb(2, fb(1, b"\x05") + fv(2, 3)))),
        ("rpu_past_32_bits", dom + desc(entry(), limit((1 << 40) | 9, 1))),
        ("empty_value", dom + desc(entry(b"k", b""), limit(3, 1))),
        ("empty_key", dom + desc(entry(b"", b"v"), limit(3, 1))),
        ("both_empty", dom + desc(entry(b"", b""), entry(), limit(3, 1))),
        ("alias_a_b_empty", dom + desc(entry(b"a_b", b""), limit(3, 1))),
        ("alias_a_b_split", dom + desc(entry(b"a", b"b"), limit(3, 1))),
        ("no_entries", dom + desc(limit(4, 2))),
        ("key_twice_value_twice", dom + desc(fb(1, fb(1, b"a") + fb(2, b"b") + fb(1, b"key_x") + fb(2, b"c")), limit(2, 2))),
        ("unit_0", dom + desc(entry(), limit(5, 0))),
        ("unit_absent", dom + desc(entry(), limit(5, None))),
        ("unit_5", dom + desc(entry(), limit(5, 5))),
        ("unit_300", dom + desc(entry(), limit(5, 300))),
        ("unit_past_32_bits", dom + desc(entry(), limit(5, (1 << 32) | 2))),
        ("four_entries", dom + desc(*[entry(b"k%d" % i, b"v%d" % i) for i in range(4)], limit(8, 4))),
        ("override_among_plain", dom + d_plain + d_ov + d_plain + desc(entry(b"z"), limit(1, 1)) + fv(3, 7)),
        ("fixed_unknown_in_descriptor", dom + desc(bytes([0x29]) + bytes(range(8)), entry(), limit(2, 1), bytes([0x2d, 1, 2, 3, 4]))),
        ("long_key_and_value", dom + desc(entry(b"K" * 300, b"V" * 5000), limit(2, 1))),
    ]


def messages():
    """-> [(label, message)]: wire_cases' ``override*`` cases, its valid messages (a fifth of their
    descriptors carry a limit, units 0..4) and the named cases above."""
    out = [("extra:" + n, m) for n, m in WC.extra_cases() if n.startswith("override")]
    out += [("valid", m) for m in WC.valid_messages()]
    out += [("named:" + n, m) for n, m in named_cases()]
    return out


def key_of(a, d):
    """descriptorKey(domain, descriptor) of descriptor d of the packer's arrays ``a`` (bytes)."""
    q = int(a["req_idx"][d])
    key = bytes(a["domain_bytes"][int(a["domain_off"][q]):int(a["domain_off"][q + 1])]) + b"."
    p = int(a["desc_off"][d])
    parts = []
    for e in range(int(a["entry_first"][d]), int(a["entry_first"][d + 1])):
        kl, vl = int(a["key_len"][e]), int(a["value_len"][e])
        k, v = bytes(a["desc_bytes"][p:p + kl]), bytes(a["desc_bytes"][p + kl + 1:p + kl + 1 + vl])
        parts.append(k + (b"_" + v if vl else b""))
        p += kl + vl + 2
    return key + b".".join(parts)


def packer_overrides(pk, msg):
    """The host packer on ``msg`` alone -> None when it is malformed, else (descriptors, [(ordinal,
    requests_per_unit, unit, key bytes)] of its descriptors with a limit, domain bytes). The key is rebuilt from the
    packer's arrays and checked against the name the packer interned (a C string: up to its first NUL)."""
    try:
        b = pk.pack([msg], [0])
    except RedisError:
        return None
    a = batch_arrays(b)
    out = []
    for d in np.nonzero(a["override_flags"])[0]:
        key = key_of(a, d)
        named = pk._lib.rl_packer_rule_key(pk.h, int(a["override_rule"][d]))
        assert named == key.split(b"\0")[0]
        out.append((int(d), int(a["override_rpu"][d]), int(a["override_unit"][d]), key))
    return b.n_descriptors, out, int(a["domain_off"][1])
