"""Serialized RateLimitRequest cases for the device parser's tests (the CPU
driver in test_wire_cpu.py, the kernels in test_gpu_wire.py), and what the
host packer, the authority, says about one message alone."""
import random

import numpy as np

from ratelimit_amd import abi
from ratelimit_amd._lib import RedisError
from ratelimit_amd.config import batch_arrays
import pbwire
from test_packer_cpu import random_requests
from test_sanitize_cpu import _malformed, _packer_inputs

ITEM_MAX = 65535  # the packed layout's per-item limits


def _entry(k=b"k", v=b"v"):
    return pbwire.field_bytes(1, (pbwire.field_bytes(1, k) if k else b"") + (pbwire.field_bytes(2, v) if v else b""))


def _desc(*entries):
    return pbwire.field_bytes(2, b"".join(entries))


def extra_cases():
    """-> [(name, message)]: wire shapes the packer accepts in ways of its own (field order and repeats,
    over-long varints, wrong wire types, fixed-width unknown fields, empty pieces, large items), and the
    packed layout's per-item limits from both sides."""
    fb, fv = pbwire.field_bytes, pbwire.field_varint
    dom = fb(1, b"domain_1")
    d1 = _desc(_entry(b"key_x", b"a_b"))
    fixed32, fixed64 = bytes([0x2d, 1, 2, 3, 4]), bytes([0x29]) + bytes(range(8))
    out = [
        ("empty", b""),
        ("domain_after_descriptors", d1 + d1 + dom),
        ("domain_twice", fb(1, b"d") + d1 + dom),
        ("hits_twice", dom + d1 + fv(3, 5) + fv(3, 9)),
        ("hits_past_32_bits", dom + d1 + fv(3, (1 << 40) | 7)),
        ("two_byte_length", dom + _desc(_entry(b"k", b"v" * 200))),
        ("overlong_varint_length", bytes([0x0a, 0x81, 0x00]) + b"d" + d1),
        ("overlong_varint_tag", bytes([0x8a, 0x00, 0x01]) + b"d" + d1),
        ("domain_as_varint", fv(1, 77) + d1),
        ("descriptors_as_fixed32", dom + bytes([0x15, 1, 2, 3, 4]) + d1),
        ("hits_as_bytes", dom + d1 + fb(3, b"\x05")),
        ("entries_as_varint", dom + fb(2, fv(1, 3) + _entry())),
        ("key_as_varint", dom + _desc(fb(1, fv(1, 9) + fb(2, b"v")))),
        ("limit_as_varint", dom + fb(2, _entry() + fv(2, 4))),
        ("fixed_unknown_in_request", fixed32 + dom + fixed64 + d1),
        ("fixed_unknown_in_descriptor", dom + fb(2, fixed64 + _entry() + fixed32)),
        ("fixed_unknown_in_entry", dom + _desc(fb(1, fixed32 + fb(1, b"k") + fixed64 + fb(2, b"v")))),
        ("descriptor_without_entries", dom + fb(2, b"") + d1),
        ("entry_empty_key", dom + _desc(_entry(b"", b"v"))),
        ("entry_empty_value", dom + _desc(_entry(b"k", b""))),
        ("entry_both_empty", dom + _desc(_entry(b"", b""), _entry())),
        ("key_twice_value_twice", dom + _desc(fb(1, fb(1, b"a") + fb(2, b"b") + fb(1, b"key_x") + fb(2, b"c")))),
        ("descriptors_300", dom + b"".join(_desc(_entry(b"k", b"%d" % i)) for i in range(300))),
        ("entries_70", dom + _desc(*[_entry(b"k%d" % i, b"v") for i in range(70)])),
        ("key_300_value_5000", dom + _desc(_entry(b"K" * 300, b"V" * 5000))),
        ("override", dom + fb(2, _entry() + fb(2, fv(1, 10) + fv(2, 1)))),
        ("override_empty", dom + d1 + fb(2, _entry() + fb(2, b""))),
        ("override_malformed", dom + fb(2, _entry() + fb(2, bytes([0x00, 0x01])))),
        ("descriptors_65535", dom + fb(2, b"") * ITEM_MAX),
        ("descriptors_65536", dom + fb(2, b"") * (ITEM_MAX + 1)),
        ("entries_65536", dom + _desc(fb(1, b"") * (ITEM_MAX + 1))),
        ("domain_65536", fb(1, b"d" * (ITEM_MAX + 1)) + d1),
        ("key_65536", dom + _desc(_entry(b"k" * (ITEM_MAX + 1), b"v"))),
        ("value_65535", dom + _desc(_entry(b"k", b"v" * ITEM_MAX))),
    ]
    return out


def valid_messages(seed=3, n=600):
    reqs = random_requests(seed, n)
    return [pbwire.encode_request(r, extra_unknown=(i % 4 == 0)) for i, r in enumerate(reqs)]


def truncations(msgs):
    return [m[:k] for m in msgs for k in range(len(m))]


def flips(n, seed=11, msgs=None):
    """n byte-flipped messages (1-3 bytes each), as test_sanitize_cpu's."""
    rng = random.Random(seed)
    msgs = [m for m in (msgs or valid_messages()) if m]
    out = []
    while len(out) < n:
        m = bytearray(rng.choice(msgs))
        for _ in range(rng.randint(1, 3)):
            m[rng.randrange(len(m))] = rng.randrange(256)
        out.append(bytes(m))
    return out


def sanitize_messages():
    """Every message of test_sanitize_cpu's packer groups, one by one."""
    return [m for msgs, _ in _packer_inputs() for m in msgs]


def malformed():
    return _malformed()


def expect(pk, msg):
    """The host packer on ``msg`` alone -> (rl_wire_status, its arrays or None)."""
    try:
        b = pk.pack([msg], [0])
    except RedisError:
        return abi.RL_WIRE_MALFORMED, None
    a = batch_arrays(b)
    per_desc = np.diff(a["entry_first"].astype(np.int64))
    if a["override_flags"].any() or b.n_descriptors > ITEM_MAX or int(a["domain_off"][-1]) > ITEM_MAX or \
            (len(per_desc) and int(per_desc.max()) > ITEM_MAX):
        return abi.RL_WIRE_DEFERRED, None
    return abi.RL_WIRE_OK, a


def arrays_fnv(a):
    """FNV-1a 64 of one OK message's arrays, in tests/c_abi/wire_parse_run.cpp's order."""
    nd, ne = len(a["req_idx"]), len(a["key_len"])
    head = np.array([nd, ne, int(a["hits"][0]), int(a["domain_off"][-1]), int(a["desc_off"][-1])], np.uint32)
    blob = b"".join(np.ascontiguousarray(x).tobytes() for x in (
        head, a["req_idx"].astype(np.uint32), a["entry_first"].astype(np.uint32), a["desc_off"].astype(np.uint32),
        a["key_len"].astype(np.uint16), a["value_len"].astype(np.uint16), a["domain_bytes"], a["desc_bytes"]))
    h = 0xcbf29ce484222325
    for b in blob:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h
