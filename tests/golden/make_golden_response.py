"""Write tests/golden/response_wire.json: serialized
envoy.service.ratelimit.v3.RateLimitResponse messages for the edge list of
tests/response_ref.py, answers -> hex.

The bytes come from the Python protobuf runtime (google.protobuf) on a
descriptor built here from the field numbers of go-control-plane v0.9.7
(rls.proto, ratelimit.proto, base.proto, duration.proto): the runtime, not the
test's own encoder, is the authority. Without the runtime the script refuses
to write. Re-run with ``python tests/golden/make_golden_response.py``.

Schema: kind "response_wire"; cases[]: descs [[code, match, requests_per_unit, unit, limit_remaining,
reset_s]..], global_shadow, keys null | [hex x 3], overall_code, headers null |
[limit, remaining, reset], hex."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import response_ref as R  # noqa: E402


def message_classes():
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name="golden_rls.proto", package="golden", syntax="proto3")

    def msg(name, fields):
        m = fd.message_type.add(name=name)
        for fname, num, typ, label, type_name in fields:
            f = m.field.add(name=fname, number=num, type=typ, label=label)
            if type_name:
                f.type_name = ".golden." + type_name

    OPT, REP = F.LABEL_OPTIONAL, F.LABEL_REPEATED
    msg("Duration", [("seconds", 1, F.TYPE_INT64, OPT, None), ("nanos", 2, F.TYPE_INT32, OPT, None)])
    msg("HeaderValue", [("key", 1, F.TYPE_STRING, OPT, None), ("value", 2, F.TYPE_STRING, OPT, None)])
    msg("RateLimit", [("requests_per_unit", 1, F.TYPE_UINT32, OPT, None), ("unit", 2, F.TYPE_INT32, OPT, None),
                      ("name", 3, F.TYPE_STRING, OPT, None)])
    msg("DescriptorStatus", [("code", 1, F.TYPE_INT32, OPT, None), ("current_limit", 2, F.TYPE_MESSAGE, OPT, "RateLimit"),
                             ("limit_remaining", 3, F.TYPE_UINT32, OPT, None),
                             ("duration_until_reset", 4, F.TYPE_MESSAGE, OPT, "Duration")])
    msg("RateLimitResponse", [("overall_code", 1, F.TYPE_INT32, OPT, None),
                              ("statuses", 2, F.TYPE_MESSAGE, REP, "DescriptorStatus"),
                              ("response_headers_to_add", 3, F.TYPE_MESSAGE, REP, "HeaderValue"),
                              ("request_headers_to_add", 4, F.TYPE_MESSAGE, REP, "HeaderValue")])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName("golden.RateLimitResponse"))


def runtime_bytes(Response, code, descs, headers, keys):
    """shouldRateLimitWorker's response (ratelimit.go:161-210) built field by field."""
    r = Response()
    r.overall_code = code
    for c, match, rpu, unit, rem, reset in descs:
        s = r.statuses.add()
        s.code = c
        if match == R.LIMIT:
            s.current_limit.requests_per_unit = rpu
            s.current_limit.unit = unit
            s.current_limit.SetInParent()
            s.duration_until_reset.seconds = reset
            s.duration_until_reset.SetInParent()
        s.limit_remaining = rem
    if keys is not None and headers is not None:
        for k, v in zip(keys, headers):
            h = r.response_headers_to_add.add()
            h.key = k.decode()
            h.value = str(v)
    return r.SerializeToString(deterministic=True)


def cases():
    out = []
    for i, descs in enumerate(R.edge_requests()):
        keys = R.KEY_SETS[i % len(R.KEY_SETS)]
        gs = bool(i % 2)
        code, headers = R.verdict_of(descs, gs)
        out.append(dict(descs=[list(d) for d in descs], global_shadow=gs,
                        keys=None if keys is None else [k.hex() for k in keys], overall_code=code,
                        headers=None if headers is None else list(headers)))
    return out


def main():
    Response = message_classes()
    cs = cases()
    assert len(cs) <= 100
    for c in cs:
        keys = None if c["keys"] is None else [bytes.fromhex(k) for k in c["keys"]]
        c["hex"] = runtime_bytes(Response, c["overall_code"], [tuple(d) for d in c["descs"]],
                                 c["headers"], keys).hex()
    with open(os.path.join(HERE, "response_wire.json"), "w") as f:
        json.dump(dict(kind="response_wire", source="google.protobuf runtime on the field numbers of go-control-plane v0.9.7", cases=cs), f,
                  indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote %d cases" % len(cs))


if __name__ == "__main__":
    main()
