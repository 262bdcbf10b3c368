"""Token constraints (logit_bias, banned / allowed tokens, min_tokens) over every public interface (CPU, tiny GPT-2):
gRPC direct and through the broker front-end, the HTTP / pub-sub reply and ``generate.py``. The fields arrive and
change the output of a prompt whose plain continuation violates them, a server launched without constraints rejects
them, and requests without the fields get what they got before."""
import json
import os
import re
import subprocess
import sys

import grpc
import pytest

from helpers import save_hf_model
from llmss_amd.engine import LLMEngine, SamplingParams, build_model
from llmss_amd.serving import grpc_api
from llmss_amd.serving.broker import PQUEUE, MemoryBroker, reply_key
from llmss_amd.serving.consumer import Consumer
from llmss_amd.serving.driver import EngineDriver
from llmss_amd.serving.grpc_api import BrokerServicer, EngineServicer, GenerateRequest, Stub, serve
from llmss_amd.utils.tokenizer import encode, load_tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT = "hello world"
NEW = 12


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gpt2tok"))
    save_hf_model("gpt2", d, vocab=101, with_tokenizer=True)
    return d


def _direct(m, tok, constraints, eos=None, **con):
    eng = LLMEngine(m, max_num_seqs=4, block_size=4, num_blocks=128, eos_token_id=eos, constraints=constraints)
    eng.add_request(encode(tok, PROMPT), SamplingParams(max_new_tokens=NEW, is_greedy=True, **con))
    while eng.has_unfinished():
        eng.step()
    return eng.pop_finished()[0].output_ids


@pytest.fixture(scope="module")
def served(model_dir):
    m = build_model(model_dir, None, "fp32", "cpu")
    tok = load_tokenizer(model_dir, m.cfg.vocab_size)
    on = EngineDriver(LLMEngine(m, max_num_seqs=8, block_size=4, num_blocks=256, eos_token_id=None,
                                constraints=True)).start()
    off = EngineDriver(LLMEngine(m, max_num_seqs=8, block_size=4, num_blocks=256, eos_token_id=None)).start()
    plain = _direct(m, tok, False)
    absent = [t for t in range(101) if t not in plain]
    # the plain continuation holds both banned tokens and not the biased one
    con = dict(logit_bias={absent[3]: 2.5, plain[-1]: -100.0}, banned_token_ids=list(dict.fromkeys(plain))[:2],
               min_tokens=3)
    want = _direct(m, tok, True, **con)
    assert want != plain and not set(con["banned_token_ids"]) & set(want) and plain[-1] not in want
    allowed = absent[5:10]
    only = _direct(m, tok, True, allowed_token_ids=allowed)
    assert set(only) <= set(allowed) and not set(plain) & set(allowed)
    yield on, off, tok, plain, want, con, allowed, only
    on.stop()
    off.stop()


def _wire(con):
    """The gRPC fields of a constraint dict."""
    d = {k: v for k, v in con.items() if k != "logit_bias"}
    if "logit_bias" in con:
        d.update(logit_bias_ids=list(con["logit_bias"]), logit_bias_values=list(con["logit_bias"].values()))
    return d


def test_grpc_direct(served):
    on, off, tok, plain, want, con, allowed, only = served
    s_on, s_off = (serve(EngineServicer(d, tok), port=0, host="127.0.0.1") for d in (on, off))
    try:
        a = Stub(grpc.insecure_channel(f"127.0.0.1:{s_on.bound_port}"))
        b = Stub(grpc.insecure_channel(f"127.0.0.1:{s_off.bound_port}"))
        base = dict(prompt=PROMPT, max_new_tokens=NEW, is_greedy=True)
        r = a.Generate(GenerateRequest(**base, **_wire(con)), timeout=60)
        assert list(r.token_ids) == want
        toks = list(a.GenerateStream(GenerateRequest(**base, **_wire(con)), timeout=60))
        assert [t.token_id for t in toks[:-1]] == want
        r = a.Generate(GenerateRequest(**base, allowed_token_ids=allowed), timeout=60)
        assert list(r.token_ids) == only
        # without the fields: the same reply from a server with and without constraints
        pa, pb = (s.Generate(GenerateRequest(**base), timeout=60) for s in (a, b))
        assert list(pa.token_ids) == plain == list(pb.token_ids)
        for m_ in (pa, pb):
            m_.ttft_s = m_.e2e_s = 0.0
        assert pa.SerializeToString() == pb.SerializeToString()
        # lengths that differ, values out of range, ids outside the vocabulary, nothing left to sample
        for bad in (dict(logit_bias_ids=[1, 2], logit_bias_values=[1.0]), dict(logit_bias_values=[1.0]),
                    dict(logit_bias_ids=[1, 1], logit_bias_values=[1.0, 2.0]),
                    dict(logit_bias_ids=[1], logit_bias_values=[101.0]), dict(banned_token_ids=[-1]),
                    dict(min_tokens=NEW + 1), dict(allowed_token_ids=[4, 4])):
            with pytest.raises(grpc.RpcError) as e:
                a.Generate(GenerateRequest(**base, **bad), timeout=10)
            assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT, bad
        for bad in (dict(banned_token_ids=[101]), dict(allowed_token_ids=[5], banned_token_ids=[5])):
            with pytest.raises(grpc.RpcError) as e:  # the engine's own range / empty-set check: the request fails
                a.Generate(GenerateRequest(**base, **bad), timeout=10)
            assert e.value.code() in (grpc.StatusCode.INVALID_ARGUMENT, grpc.StatusCode.UNAVAILABLE)
        assert list(a.Generate(GenerateRequest(**base), timeout=60).token_ids) == plain  # still serving
        # a server launched without constraints
        for call in (lambda: b.Generate(GenerateRequest(**base, **_wire(con)), timeout=10),
                     lambda: list(b.GenerateStream(GenerateRequest(**base, min_tokens=2), timeout=10)),
                     lambda: b.Generate(GenerateRequest(**base, banned_token_ids=[3]), timeout=10),
                     lambda: b.Generate(GenerateRequest(**base, allowed_token_ids=[3]), timeout=10)):
            with pytest.raises(grpc.RpcError) as e:
                call()
            assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
            assert "--constraints" in e.value.details()
        assert list(b.Generate(GenerateRequest(**base, min_tokens=0), timeout=60).token_ids) == plain
    finally:
        s_on.stop(0)
        s_off.stop(0)


def test_http_pubsub_and_broker_front_end(served):
    from fastapi.testclient import TestClient

    from llmss_amd.serving.producer import create_app

    on, off, tok, plain, want, con, allowed, only = served
    body = {"prompt": PROMPT, "max_new_tokens": NEW, "is_greedy": True, "temperature": 1.0, "top_p": 0.95, "top_k": 50}
    # as a JSON client sends it: the keys of logit_bias are strings
    jcon = json.loads(json.dumps({**con, "logit_bias": {str(k): v for k, v in con["logit_bias"].items()}}))
    assert all(isinstance(k, str) for k in jcon["logit_bias"])
    replies = {}
    for name, drv in (("on", on), ("off", off)):
        b = MemoryBroker()
        consumer = Consumer(drv, tok, b, poll_timeout=0.2).start()
        try:
            client = TestClient(create_app(b, timeout_s=60))
            p = client.post("/generate", json=body)
            assert p.status_code == 200
            replies[name] = json.loads(p.content)
            b.lpush(PQUEUE, json.dumps({**body, "request_id": "plain"}))
            replies[name + "-raw"] = json.loads(b.brpop(reply_key("plain"), 30))
            b.lpush(PQUEUE, json.dumps({**body, "request_id": "con", **jcon}))
            rep = json.loads(b.brpop(reply_key("con"), 30))
            if name == "off":  # an error reply, and the consumer keeps serving
                assert "error" in rep
                b.lpush(PQUEUE, json.dumps({**body, "request_id": "again"}))
                assert json.loads(b.brpop(reply_key("again"), 30))["continuation"] == tok.decode(plain)
                continue
            assert "error" not in rep and rep["continuation"] == tok.decode(want)
            assert rep["continuation"] != replies["on"]["continuation"]
            assert client.post("/generate", json={**body, **jcon}).json()["continuation"] == rep["continuation"]
            b.lpush(PQUEUE, json.dumps({**body, "request_id": "int-keys", **con}))  # json.dumps turns them into strings
            assert json.loads(b.brpop(reply_key("int-keys"), 30))["continuation"] == rep["continuation"]
            b.lpush(PQUEUE, json.dumps({**body, "request_id": "allow", "allowed_token_ids": allowed}))
            assert json.loads(b.brpop(reply_key("allow"), 30))["continuation"] == tok.decode(only)
            for i, bad in enumerate(({"logit_bias": {"7": 500}}, {"logit_bias": {"x": 1}}, {"banned_token_ids": [101]},
                                     {"min_tokens": NEW + 1})):
                b.lpush(PQUEUE, json.dumps({**body, "request_id": f"bad{i}", **bad}))
                assert "error" in json.loads(b.brpop(reply_key(f"bad{i}"), 30)), bad
            fe = serve(BrokerServicer(b), port=0, host="127.0.0.1")
            try:
                stub = Stub(grpc.insecure_channel(f"127.0.0.1:{fe.bound_port}"))
                base = dict(prompt=PROMPT, max_new_tokens=NEW, is_greedy=True)
                g = stub.Generate(GenerateRequest(**base, **_wire(con)), timeout=60)
                assert g.continuation == tok.decode(want)
                toks = list(stub.GenerateStream(GenerateRequest(**base, **_wire(con)), timeout=60))
                assert [t.token_id for t in toks[:-1]] == want
                g = stub.Generate(GenerateRequest(**base, allowed_token_ids=allowed), timeout=60)
                assert g.continuation == tok.decode(only)
                z = stub.Generate(GenerateRequest(**base), timeout=60)
                assert z.continuation == tok.decode(plain)
                with pytest.raises(grpc.RpcError) as e:
                    stub.Generate(GenerateRequest(**base, logit_bias_ids=[1, 2], logit_bias_values=[1.0]), timeout=10)
                assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
            finally:
                fe.stop(0)
        finally:
            consumer.stop()
    varies = {"ttft_s", "e2e_s"}
    strip = lambda d: {k: v for k, v in d.items() if k not in varies}  # noqa: E731
    assert replies["on"].pop("request_id") != replies["off"].pop("request_id")  # the producer's random ids
    assert strip(replies["on"]) == strip(replies["off"]) and replies["on"]["continuation"] == tok.decode(plain)
    assert strip(replies["on-raw"]) == strip(replies["off-raw"])
    assert not {"logit_bias", "banned_token_ids", "allowed_token_ids", "min_tokens"} & set(replies["on-raw"])


def _cli(model_dir, *extra):
    r = subprocess.run([sys.executable, "generate.py", "--pretrained_model_path", model_dir, "--prompts", PROMPT,
                        "--max_new_tokens", str(NEW), "--is_greedy", "--device", "cpu", *extra],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("cache", [[], ["--use_cache"]])
def test_generate_cli(served, model_dir, cache):
    on, off, tok, plain, want, con, allowed, only = served
    flags = ["--logit_bias", json.dumps({str(k): v for k, v in con["logit_bias"].items()}), "--banned_token_ids",
             *map(str, con["banned_token_ids"]), "--min_tokens", str(con["min_tokens"])]
    base = _cli(model_dir, *cache)
    same = _cli(model_dir, *cache, "--min_tokens", "0", "--logit_bias", "{}")
    got = _cli(model_dir, *cache, *flags)
    allow = _cli(model_dir, *cache, "--allowed_token_ids", *map(str, allowed))
    assert len(base) == 4 and base[1:3] == same[1:3]  # lines 0 and 3 carry times
    assert [re.sub(r"[0-9.]+", "#", ln) for ln in base] == [re.sub(r"[0-9.]+", "#", ln) for ln in same]
    eos = tok.eos_token_id  # the CLI stops at the tokenizer's EOS, so the runs to compare with know it too
    m = on.engine.model
    assert base[2] == f"continuations: {[tok.decode(_direct(m, tok, False, eos=eos))]}"
    assert got[2] == f"continuations: {[tok.decode(_direct(m, tok, True, eos=eos, **con))]}" and got[2] != base[2]
    assert allow[2] == f"continuations: {[tok.decode(_direct(m, tok, True, eos=eos, allowed_token_ids=allowed))]}"
    assert allow[2] not in (base[2], got[2])


def test_proto_and_launch_flag():
    import argparse

    from llmss_amd.serving.launch import add_engine_args

    req = grpc_api._POOL.FindMessageTypeByName("llmss.GenerateRequest")
    F = grpc_api._F
    fields = (("logit_bias_ids", 16, "int32", True), ("logit_bias_values", 17, "float", True),
              ("banned_token_ids", 18, "int32", True), ("allowed_token_ids", 19, "int32", True),
              ("min_tokens", 20, "int32", False))
    text = open(os.path.join(ROOT, "proto", "generate.proto")).read()
    for name, num, typ, rep in fields:
        f = req.fields_by_name[name]
        assert f.number == num and f.type == (F.TYPE_FLOAT if typ == "float" else F.TYPE_INT32)
        assert hasattr(getattr(GenerateRequest(), name), "append") == rep  # a repeated field
        assert re.search(rf"{'repeated ' if rep else ''}{typ}\s+{name}\s*=\s*{num}\s*;", text)
    p = add_engine_args(argparse.ArgumentParser())
    assert p.parse_args([]).constraints is False and p.parse_args(["--constraints"]).constraints is True
