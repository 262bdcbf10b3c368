"""min_p over every public interface (CPU, tiny GPT-2): gRPC field 21 direct and through the broker front-end, the
HTTP / pub-sub key, ``generate.py --min_p`` and ``--min-p`` on the launcher. The field arrives and changes the output of
a seeded request, a server launched without min-p rejects it, and requests without it get what they got before."""
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
# the tiny model's logits span less than a nat: temperature 0.2 spreads the scaled ones enough for a floor to bite
SAMPLED = dict(temperature=0.2, top_p=1.0, top_k=60, seed=5)
MIN_P = 0.3


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gpt2tok"))
    save_hf_model("gpt2", d, vocab=101, with_tokenizer=True)
    return d


def _direct(m, tok, on, eos=None, **kw):
    eng = LLMEngine(m, max_num_seqs=4, block_size=4, num_blocks=128, eos_token_id=eos, min_p=on)
    eng.add_request(encode(tok, PROMPT), SamplingParams(max_new_tokens=NEW, **SAMPLED, **kw))
    while eng.has_unfinished():
        eng.step()
    return eng.pop_finished()[0].output_ids


@pytest.fixture(scope="module")
def served(model_dir):
    m = build_model(model_dir, None, "fp32", "cpu")
    tok = load_tokenizer(model_dir, m.cfg.vocab_size)
    on = EngineDriver(LLMEngine(m, max_num_seqs=8, block_size=4, num_blocks=256, eos_token_id=None,
                                min_p=True)).start()
    off = EngineDriver(LLMEngine(m, max_num_seqs=8, block_size=4, num_blocks=256, eos_token_id=None)).start()
    plain = _direct(m, tok, False)
    want = _direct(m, tok, True, min_p=MIN_P)
    assert want != plain and _direct(m, tok, True) == plain
    yield on, off, tok, plain, want
    on.stop()
    off.stop()


def test_grpc_direct(served):
    on, off, tok, plain, want = served
    s_on, s_off = (serve(EngineServicer(d, tok), port=0, host="127.0.0.1") for d in (on, off))
    try:
        a = Stub(grpc.insecure_channel(f"127.0.0.1:{s_on.bound_port}"))
        b = Stub(grpc.insecure_channel(f"127.0.0.1:{s_off.bound_port}"))
        base = dict(prompt=PROMPT, max_new_tokens=NEW, **SAMPLED)
        r = a.Generate(GenerateRequest(**base, min_p=MIN_P), timeout=60)
        assert list(r.token_ids) == want
        toks = list(a.GenerateStream(GenerateRequest(**base, min_p=MIN_P), timeout=60))
        assert [t.token_id for t in toks[:-1]] == want
        # without the field, and with 0 (unset on the wire): the same reply from a server with and without min-p
        pa, pb = (s.Generate(GenerateRequest(**base), timeout=60) for s in (a, b))
        assert list(pa.token_ids) == plain == list(pb.token_ids)
        for m_ in (pa, pb):
            m_.ttft_s = m_.e2e_s = 0.0
        assert pa.SerializeToString() == pb.SerializeToString()
        assert list(a.Generate(GenerateRequest(**base, min_p=0.0), timeout=60).token_ids) == plain
        for bad in (1.5, -0.1, float("nan"), float("inf")):
            with pytest.raises(grpc.RpcError) as e:
                a.Generate(GenerateRequest(**base, min_p=bad), timeout=10)
            assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT, bad
            assert "min_p" in e.value.details()
        assert list(a.Generate(GenerateRequest(**base), timeout=60).token_ids) == plain  # still serving
        # a server launched without min-p
        for call in (lambda: b.Generate(GenerateRequest(**base, min_p=MIN_P), timeout=10),
                     lambda: list(b.GenerateStream(GenerateRequest(**base, min_p=1.0), timeout=10))):
            with pytest.raises(grpc.RpcError) as e:
                call()
            assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
            assert "--min-p" in e.value.details()
        assert list(b.Generate(GenerateRequest(**base, min_p=0.0), timeout=60).token_ids) == plain
    finally:
        s_on.stop(0)
        s_off.stop(0)


def test_http_pubsub_and_broker_front_end(served):
    from fastapi.testclient import TestClient

    from llmss_amd.serving.producer import create_app

    on, off, tok, plain, want = served
    body = {"prompt": PROMPT, "max_new_tokens": NEW, "is_greedy": False, **SAMPLED}
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
            b.lpush(PQUEUE, json.dumps({**body, "request_id": "floor", "min_p": MIN_P}))
            rep = json.loads(b.brpop(reply_key("floor"), 30))
            if name == "off":  # an error reply, and the consumer keeps serving
                assert "error" in rep and "min_p" in rep["error"]
                b.lpush(PQUEUE, json.dumps({**body, "request_id": "again", "min_p": 0.0}))
                assert json.loads(b.brpop(reply_key("again"), 30))["continuation"] == tok.decode(plain)
                continue
            assert "error" not in rep and rep["continuation"] == tok.decode(want)
            assert rep["continuation"] != replies["on"]["continuation"]
            assert client.post("/generate", json={**body, "min_p": MIN_P}).json()["continuation"] == rep["continuation"]
            for i, bad in enumerate((1.5, -1, "a lot")):
                b.lpush(PQUEUE, json.dumps({**body, "request_id": f"bad{i}", "min_p": bad}))
                assert "error" in json.loads(b.brpop(reply_key(f"bad{i}"), 30)), bad
            fe = serve(BrokerServicer(b), port=0, host="127.0.0.1")
            try:
                stub = Stub(grpc.insecure_channel(f"127.0.0.1:{fe.bound_port}"))
                base = dict(prompt=PROMPT, max_new_tokens=NEW, **SAMPLED)
                g = stub.Generate(GenerateRequest(**base, min_p=MIN_P), timeout=60)
                assert g.continuation == tok.decode(want)
                toks = list(stub.GenerateStream(GenerateRequest(**base, min_p=MIN_P), timeout=60))
                assert [t.token_id for t in toks[:-1]] == want
                z = stub.Generate(GenerateRequest(**base), timeout=60)
                assert z.continuation == tok.decode(plain)
            finally:
                fe.stop(0)
        finally:
            consumer.stop()
    varies = {"ttft_s", "e2e_s"}
    strip = lambda d: {k: v for k, v in d.items() if k not in varies}  # noqa: E731
    assert replies["on"].pop("request_id") != replies["off"].pop("request_id")  # the producer's random ids
    assert strip(replies["on"]) == strip(replies["off"]) and replies["on"]["continuation"] == tok.decode(plain)
    assert strip(replies["on-raw"]) == strip(replies["off-raw"]) and "min_p" not in replies["on-raw"]


def _cli(model_dir, *extra):
    r = subprocess.run([sys.executable, "generate.py", "--pretrained_model_path", model_dir, "--prompts", PROMPT,
                        "--max_new_tokens", str(NEW), "--temperature", str(SAMPLED["temperature"]), "--top_p", "1.0",
                        "--top_k", str(SAMPLED["top_k"]), "--seed", str(SAMPLED["seed"]), "--device", "cpu", *extra],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("cache", [[], ["--use_cache"]])
def test_generate_cli(served, model_dir, cache):
    on, off, tok, plain, want = served
    base = _cli(model_dir, *cache)
    same = _cli(model_dir, *cache, "--min_p", "0")
    got = _cli(model_dir, *cache, "--min_p", str(MIN_P))
    assert len(base) == 4 and base[1:3] == same[1:3]  # lines 0 and 3 carry times
    assert [re.sub(r"[0-9.]+", "#", ln) for ln in base] == [re.sub(r"[0-9.]+", "#", ln) for ln in same]
    eos = tok.eos_token_id  # the CLI stops at the tokenizer's EOS, so the runs to compare with know it too
    m = on.engine.model
    assert base[2] == f"continuations: {[tok.decode(_direct(m, tok, False, eos=eos))]}"
    assert got[2] == f"continuations: {[tok.decode(_direct(m, tok, True, eos=eos, min_p=MIN_P))]}" and got[2] != base[2]
    r = subprocess.run([sys.executable, "generate.py", "--pretrained_model_path", model_dir, "--prompts", PROMPT,
                        "--device", "cpu", "--min_p", "1.5"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "min_p" in r.stderr


def test_proto_and_launch_flag():
    import argparse

    from llmss_amd.serving.launch import add_engine_args

    f = grpc_api._POOL.FindMessageTypeByName("llmss.GenerateRequest").fields_by_name["min_p"]
    assert f.number == 21 and f.type == grpc_api._F.TYPE_FLOAT
    assert GenerateRequest().min_p == 0.0  # unset is off
    text = open(os.path.join(ROOT, "proto", "generate.proto")).read()
    assert re.search(r"float\s+min_p\s*=\s*21\s*;", text)
    p = add_engine_args(argparse.ArgumentParser())
    assert p.parse_args([]).min_p is False and p.parse_args(["--min-p"]).min_p is True
    from llmss_amd.serving.protocol import parse_request, to_sampling

    assert to_sampling(parse_request(json.dumps({"prompt": "x"}))).min_p == 0.0
    assert to_sampling(parse_request(json.dumps({"prompt": "x", "min_p": 0.25}))).min_p == 0.25
