"""Repetition / presence / frequency penalties over every public interface (CPU, tiny GPT-2): gRPC direct and through
the broker front-end, the HTTP / pub-sub reply and ``generate.py``. The fields arrive and change the output of a
prompt whose plain continuation repeats itself, repetition_penalty = 0 means 1.0 on the wire, a server launched
without penalties rejects them, and requests without the fields get what they got before."""
import json
import os
import re
import struct
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
PEN = dict(repetition_penalty=1.5, presence_penalty=1.0, frequency_penalty=0.5)


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gpt2tok"))
    save_hf_model("gpt2", d, vocab=101, with_tokenizer=True)
    return d


def _direct(m, tok, penalties, **pen):
    eng = LLMEngine(m, max_num_seqs=4, block_size=4, num_blocks=128, eos_token_id=None, penalties=penalties)
    eng.add_request(encode(tok, PROMPT), SamplingParams(max_new_tokens=NEW, is_greedy=True, **pen))
    while eng.has_unfinished():
        eng.step()
    return eng.pop_finished()[0].output_ids


@pytest.fixture(scope="module")
def served(model_dir):
    m = build_model(model_dir, None, "fp32", "cpu")
    tok = load_tokenizer(model_dir, m.cfg.vocab_size)
    on = EngineDriver(LLMEngine(m, max_num_seqs=8, block_size=4, num_blocks=256, eos_token_id=None,
                                penalties=True)).start()
    off = EngineDriver(LLMEngine(m, max_num_seqs=8, block_size=4, num_blocks=256, eos_token_id=None)).start()
    plain = _direct(m, tok, False)
    # what a proto `float` field carries of the penalties
    want = _direct(m, tok, True, **{k: f32(v) for k, v in PEN.items()})
    assert len(set(plain)) < len(plain), "the plain continuation does not repeat: the test shows nothing"
    assert want != plain
    yield on, off, tok, plain, want
    on.stop()
    off.stop()


def test_grpc_direct(served):
    on, off, tok, plain, want = served
    s_on, s_off = (serve(EngineServicer(d, tok), port=0, host="127.0.0.1") for d in (on, off))
    try:
        a = Stub(grpc.insecure_channel(f"127.0.0.1:{s_on.bound_port}"))
        b = Stub(grpc.insecure_channel(f"127.0.0.1:{s_off.bound_port}"))
        base = dict(prompt=PROMPT, max_new_tokens=NEW, is_greedy=True)
        r = a.Generate(GenerateRequest(**base, **PEN), timeout=60)
        assert list(r.token_ids) == want
        toks = list(a.GenerateStream(GenerateRequest(**base, **PEN), timeout=60))
        assert [t.token_id for t in toks[:-1]] == want
        # repetition_penalty = 0 (unset on the wire) means 1.0: with the other two unset, no penalty at all
        z = a.Generate(GenerateRequest(**base, repetition_penalty=0.0), timeout=60)
        assert list(z.token_ids) == plain
        only_pf = a.Generate(GenerateRequest(**base, presence_penalty=1.0, frequency_penalty=0.5), timeout=60)
        assert list(only_pf.token_ids) == _direct(on.engine.model, tok, True, presence_penalty=1.0,
                                                  frequency_penalty=0.5)
        # without the fields: the same reply from a server with and without penalties
        pa, pb = (s.Generate(GenerateRequest(**base), timeout=60) for s in (a, b))
        assert list(pa.token_ids) == plain == list(pb.token_ids)
        for m_ in (pa, pb):
            m_.ttft_s = m_.e2e_s = 0.0
        assert pa.SerializeToString() == pb.SerializeToString()
        # out of range, and a server launched without penalties
        for bad in (dict(presence_penalty=2.5), dict(frequency_penalty=-3.0), dict(repetition_penalty=-1.0)):
            with pytest.raises(grpc.RpcError) as e:
                a.Generate(GenerateRequest(**base, **bad), timeout=10)
            assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
        for call in (lambda: b.Generate(GenerateRequest(**base, **PEN), timeout=10),
                     lambda: list(b.GenerateStream(GenerateRequest(**base, frequency_penalty=0.5), timeout=10))):
            with pytest.raises(grpc.RpcError) as e:
                call()
            assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
        assert list(b.Generate(GenerateRequest(**base, repetition_penalty=1.0), timeout=60).token_ids) == plain
    finally:
        s_on.stop(0)
        s_off.stop(0)


def test_http_pubsub_and_broker_front_end(served):
    from fastapi.testclient import TestClient

    from llmss_amd.serving.producer import create_app

    on, off, tok, plain, want = served
    body = {"prompt": PROMPT, "max_new_tokens": NEW, "is_greedy": True, "temperature": 1.0, "top_p": 0.95, "top_k": 50}
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
            b.lpush(PQUEUE, json.dumps({**body, "request_id": "pen", **PEN}))
            rep = json.loads(b.brpop(reply_key("pen"), 30))
            if name == "off":  # an error reply, and the consumer keeps serving
                assert "error" in rep
                b.lpush(PQUEUE, json.dumps({**body, "request_id": "again"}))
                assert json.loads(b.brpop(reply_key("again"), 30))["continuation"] == tok.decode(plain)
                continue
            assert "error" not in rep and rep["continuation"] == tok.decode(_direct(on.engine.model, tok, True, **PEN))
            assert rep["continuation"] != replies["on"]["continuation"]
            assert client.post("/generate", json={**body, **PEN}).json()["continuation"] == rep["continuation"]
            b.lpush(PQUEUE, json.dumps({**body, "request_id": "bad", "presence_penalty": 9}))
            assert "error" in json.loads(b.brpop(reply_key("bad"), 30))
            fe = serve(BrokerServicer(b), port=0, host="127.0.0.1")
            try:
                stub = Stub(grpc.insecure_channel(f"127.0.0.1:{fe.bound_port}"))
                g = stub.Generate(GenerateRequest(prompt=PROMPT, max_new_tokens=NEW, is_greedy=True, **PEN), timeout=60)
                assert g.continuation == tok.decode(want)
                z = stub.Generate(GenerateRequest(prompt=PROMPT, max_new_tokens=NEW, is_greedy=True), timeout=60)
                assert z.continuation == tok.decode(plain)
            finally:
                fe.stop(0)
        finally:
            consumer.stop()
    varies = {"ttft_s", "e2e_s"}
    strip = lambda d: {k: v for k, v in d.items() if k not in varies}  # noqa: E731
    assert replies["on"].pop("request_id") != replies["off"].pop("request_id")  # the producer's random ids
    assert strip(replies["on"]) == strip(replies["off"]) and replies["on"]["continuation"] == tok.decode(plain)
    assert strip(replies["on-raw"]) == strip(replies["off-raw"])
    assert not {"repetition_penalty", "presence_penalty", "frequency_penalty"} & set(replies["on-raw"])


def _cli(model_dir, *extra):
    r = subprocess.run([sys.executable, "generate.py", "--pretrained_model_path", model_dir, "--prompts", PROMPT,
                        "--max_new_tokens", str(NEW), "--is_greedy", "--device", "cpu", *extra],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("cache", [[], ["--use_cache"]])
def test_generate_cli(served, model_dir, cache):
    on, off, tok, plain, want = served
    flags = [x for k, v in PEN.items() for x in (f"--{k}", str(v))]
    base = _cli(model_dir, *cache)
    same = _cli(model_dir, *cache, "--repetition_penalty", "1.0", "--presence_penalty", "0", "--frequency_penalty", "0")
    pen = _cli(model_dir, *cache, *flags)
    assert len(base) == 4 and base[1:3] == same[1:3]  # lines 0 and 3 carry times
    assert [re.sub(r"[0-9.]+", "#", ln) for ln in base] == [re.sub(r"[0-9.]+", "#", ln) for ln in same]
    # the CLI stops at the tokenizer's EOS, the engine runs of the fixture do not: compare up to it
    eos = tok.eos_token_id

    def cut(ids):
        return ids[:ids.index(eos) + 1] if eos in ids else ids
    assert base[2] == f"continuations: {[tok.decode(cut(plain))]}"
    exact = _direct(on.engine.model, tok, True, **PEN)
    assert pen[2] == f"continuations: {[tok.decode(cut(exact))]}" and pen[2] != base[2]


def test_proto_and_launch_flag():
    import argparse

    from llmss_amd.serving.launch import add_engine_args

    req = grpc_api._POOL.FindMessageTypeByName("llmss.GenerateRequest")
    F = grpc_api._F
    for name, num in (("repetition_penalty", 13), ("presence_penalty", 14), ("frequency_penalty", 15)):
        f = req.fields_by_name[name]
        assert f.number == num and f.type == F.TYPE_FLOAT
    text = open(os.path.join(ROOT, "proto", "generate.proto")).read()
    for name, num in (("repetition_penalty", 13), ("presence_penalty", 14), ("frequency_penalty", 15)):
        assert re.search(rf"float\s+{name}\s*=\s*{num}\s*;", text)
    p = add_engine_args(argparse.ArgumentParser())
    assert p.parse_args([]).penalties is False and p.parse_args(["--penalties"]).penalties is True
