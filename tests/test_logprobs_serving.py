"""Log-probabilities over every public interface (CPU, tiny GPT-2): gRPC unary and stream, the HTTP / pub-sub final
reply and ``generate.py --logprobs`` carry the engine's numbers; requests without the option get replies without
the new fields; the .proto file and the hand-built descriptor agree."""
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
from llmss_amd.serving.broker import MemoryBroker
from llmss_amd.serving.consumer import Consumer
from llmss_amd.serving.driver import EngineDriver
from llmss_amd.serving.grpc_api import BrokerServicer, EngineServicer, GenerateRequest, Stub, serve
from llmss_amd.utils.tokenizer import encode, load_tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROMPT = "hello world"
NEW = 6


def f32(x):
    """A Python float as the fp32 value it is carried as in a proto `float` field."""
    return struct.unpack("<f", struct.pack("<f", x))[0]


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gpt2tok"))
    save_hf_model("gpt2", d, vocab=101, with_tokenizer=True)
    return d


@pytest.fixture(scope="module")
def served(model_dir):
    m = build_model(model_dir, None, "fp32", "cpu")
    tok = load_tokenizer(model_dir, m.cfg.vocab_size)
    drv = EngineDriver(LLMEngine(m, max_num_seqs=8, block_size=4, num_blocks=256, eos_token_id=None,
                                 max_logprobs=5)).start()
    # the engine's own numbers, from an engine of its own
    eng = LLMEngine(m, max_num_seqs=4, block_size=4, num_blocks=128, eos_token_id=None, max_logprobs=5)
    eng.add_request(encode(tok, PROMPT), SamplingParams(max_new_tokens=NEW, is_greedy=True, logprobs=3))
    while eng.has_unfinished():
        eng.step()
    want = eng.pop_finished()[0]
    assert len(want.output_logprobs) == NEW and all(len(t) == 3 for t in want.output_top_logprobs)
    yield drv, tok, m, want
    drv.stop()


def _same_top(msg, top):
    assert list(msg.token_ids) == [i for i, _ in top]
    assert list(msg.logprobs) == [f32(v) for _, v in top]


def test_grpc_unary_and_stream(served):
    drv, tok, m, want = served
    server = serve(EngineServicer(drv, tok), port=0, host="127.0.0.1")
    try:
        stub = Stub(grpc.insecure_channel(f"127.0.0.1:{server.bound_port}"))
        req = GenerateRequest(prompt=PROMPT, max_new_tokens=NEW, is_greedy=True, return_logprobs=True, top_logprobs=3)
        r = stub.Generate(req, timeout=60)
        assert list(r.token_ids) == want.output_ids
        assert list(r.token_logprobs) == [f32(v) for v in want.output_logprobs]
        assert len(r.top_logprobs) == NEW
        for msg, top in zip(r.top_logprobs, want.output_top_logprobs):
            _same_top(msg, top)
        toks = list(stub.GenerateStream(req, timeout=60))
        assert toks[-1].finished and not toks[-1].HasField("top")
        assert [t.token_id for t in toks[:-1]] == want.output_ids
        for t, lp, top in zip(toks[:-1], want.output_logprobs, want.output_top_logprobs):
            assert t.HasField("top") and t.logprob == f32(lp)
            _same_top(t.top, top)
        # the token's log-probability alone
        r0 = stub.Generate(GenerateRequest(prompt=PROMPT, max_new_tokens=NEW, is_greedy=True, return_logprobs=True),
                           timeout=60)
        assert list(r0.token_logprobs) == list(r.token_logprobs)
        assert len(r0.top_logprobs) == NEW and all(len(t.token_ids) == 0 for t in r0.top_logprobs)
        # without the option: no new fields (top_logprobs alone does not ask)
        for plain in (GenerateRequest(prompt=PROMPT, max_new_tokens=NEW, is_greedy=True),
                      GenerateRequest(prompt=PROMPT, max_new_tokens=NEW, is_greedy=True, top_logprobs=3)):
            p = stub.Generate(plain, timeout=60)
            assert list(p.token_ids) == want.output_ids and not p.token_logprobs and not p.top_logprobs
            ts = list(stub.GenerateStream(plain, timeout=60))
            assert all(not t.HasField("top") and t.logprob == 0.0 for t in ts)
        # not served: more alternatives than the engine computes, or out of range
        for n in (6, 21):
            with pytest.raises(grpc.RpcError) as e:
                stub.Generate(GenerateRequest(prompt=PROMPT, max_new_tokens=2, return_logprobs=True, top_logprobs=n),
                              timeout=10)
            assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
            with pytest.raises(grpc.RpcError) as e:
                list(stub.GenerateStream(GenerateRequest(prompt=PROMPT, max_new_tokens=2, return_logprobs=True,
                                                         top_logprobs=n), timeout=10))
            assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    finally:
        server.stop(0)


def test_grpc_rejects_logprobs_on_a_server_without_them(model_dir):
    m = build_model(model_dir, None, "fp32", "cpu")
    tok = load_tokenizer(model_dir, m.cfg.vocab_size)
    drv = EngineDriver(LLMEngine(m, max_num_seqs=4, block_size=4, num_blocks=64, eos_token_id=None)).start()
    server = serve(EngineServicer(drv, tok), port=0, host="127.0.0.1")
    try:
        stub = Stub(grpc.insecure_channel(f"127.0.0.1:{server.bound_port}"))
        with pytest.raises(grpc.RpcError) as e:
            stub.Generate(GenerateRequest(prompt=PROMPT, max_new_tokens=2, return_logprobs=True), timeout=10)
        assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
        assert len(stub.Generate(GenerateRequest(prompt=PROMPT, max_new_tokens=2, is_greedy=True),
                                 timeout=60).token_ids) == 2
    finally:
        server.stop(0)
        drv.stop()


def test_http_pubsub_final_reply(served):
    from fastapi.testclient import TestClient

    from llmss_amd.serving.producer import create_app

    drv, tok, m, want = served
    b = MemoryBroker()
    consumer = Consumer(drv, tok, b, poll_timeout=0.2).start()
    try:
        client = TestClient(create_app(b, timeout_s=60))
        body = {"prompt": PROMPT, "max_new_tokens": NEW, "is_greedy": True, "temperature": 1.0, "top_p": 0.95,
                "top_k": 50}
        r = client.post("/generate", json={**body, "logprobs": 3})
        assert r.status_code == 200
        d = r.json()
        assert d["token_logprobs"] == want.output_logprobs  # JSON carries the doubles exactly
        assert d["top_logprobs"] == [[[i, v] for i, v in top] for top in want.output_top_logprobs]
        plain = client.post("/generate", json=body)
        assert plain.status_code == 200
        raw = json.loads(plain.content)
        assert raw["continuation"] == d["continuation"]
        assert not raw.get("token_logprobs") and not raw.get("top_logprobs")
        # the broker reply itself omits the keys; a reference producer that ignores unknown keys still interoperates
        from llmss_amd.serving.broker import PQUEUE, reply_key

        b.lpush(PQUEUE, json.dumps({**body, "request_id": "plain"}))
        assert not {"token_logprobs", "top_logprobs"} & set(json.loads(b.brpop(reply_key("plain"), 30)))
        b.lpush(PQUEUE, json.dumps({**body, "request_id": "lp", "logprobs": 0}))
        rep = json.loads(b.brpop(reply_key("lp"), 30))
        assert rep["token_logprobs"] == want.output_logprobs and rep["top_logprobs"] == [[]] * NEW
        # the gRPC front-end of the pub/sub path hands them through
        fe = serve(BrokerServicer(b), port=0, host="127.0.0.1")
        try:
            stub = Stub(grpc.insecure_channel(f"127.0.0.1:{fe.bound_port}"))
            g = stub.Generate(GenerateRequest(prompt=PROMPT, max_new_tokens=NEW, is_greedy=True, return_logprobs=True,
                                              top_logprobs=3), timeout=60)
            assert list(g.token_logprobs) == [f32(v) for v in want.output_logprobs]
            for msg, top in zip(g.top_logprobs, want.output_top_logprobs):
                _same_top(msg, top)
        finally:
            fe.stop(0)
        # a request the engine cannot serve: an error reply, and the consumer keeps serving
        b.lpush(PQUEUE, json.dumps({**body, "request_id": "many", "logprobs": 6}))
        assert "error" in json.loads(b.brpop(reply_key("many"), 30))
        b.lpush(PQUEUE, json.dumps({**body, "request_id": "bad", "logprobs": 21}))
        assert "error" in json.loads(b.brpop(reply_key("bad"), 30))
    finally:
        consumer.stop()


def _cli(model_dir, *extra):
    r = subprocess.run([sys.executable, "generate.py", "--pretrained_model_path", model_dir, "--prompts", PROMPT,
                        "--max_new_tokens", str(NEW), "--is_greedy", "--device", "cpu", *extra],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("cache", [[], ["--use_cache"]])
def test_generate_cli(served, model_dir, cache):
    drv, tok, m, want = served
    plain = _cli(model_dir, *cache)
    lines = _cli(model_dir, *cache, "--logprobs", "3")
    assert not any(ln.startswith("logprobs: ") for ln in plain)
    # the reference's lines and the throughput line come first, unchanged in form; then one line per token
    assert len(plain) == 4 and plain[1:3] == lines[1:3]
    assert [re.sub(r"[0-9.]+", "#", ln) for ln in plain] == [re.sub(r"[0-9.]+", "#", ln) for ln in lines[:4]]
    got = [json.loads(ln[len("logprobs: "):]) for ln in lines[4:]]
    assert all(ln.startswith("logprobs: ") for ln in lines[4:])
    # the CLI stops at the tokenizer's EOS, the engine run above does not
    assert len(got) == NEW or (got and got[-1]["token_id"] == tok.eos_token_id)
    assert [g["token_id"] for g in got] == want.output_ids[:len(got)]
    for t, (g, lp, top) in enumerate(zip(got, want.output_logprobs, want.output_top_logprobs)):
        assert g["prompt"] == 0 and g["position"] == t and g["text"] == tok.decode([g["token_id"]])
        assert [a[0] for a in g["top"]] == [i for i, _ in top]
        if cache:  # the same engine steps: the same numbers
            assert g["logprob"] == lp and [a[2] for a in g["top"]] == [v for _, v in top]
        else:  # recompute mode re-runs the prefix as one prefill: the facade parity tests' 1e-4 on fp32 logits
            assert abs(g["logprob"] - lp) <= 1e-4 and all(abs(a[2] - v) <= 1e-4 for a, (_, v) in zip(g["top"], top))


def test_proto_file_matches_descriptor():
    """Every message of proto/generate.proto: field names, numbers, types and labels equal the descriptor's."""
    text = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "proto", "generate.proto")).read())
    F = grpc_api._F
    scalar = {"string": F.TYPE_STRING, "int32": F.TYPE_INT32, "int64": F.TYPE_INT64, "bool": F.TYPE_BOOL,
              "float": F.TYPE_FLOAT}
    seen = {}
    for name, body in re.findall(r"message\s+(\w+)\s*\{([^}]*)\}", text):
        seen[name] = [(fname, int(num), ftype, bool(rep))
                      for rep, ftype, fname, num in re.findall(r"(repeated\s+)?(\w+)\s+(\w+)\s*=\s*(\d+)\s*;", body)]
    assert {"GenerateRequest", "GenerateResponse", "Token", "TopLogprobs"} <= set(seen)
    for name, fields in seen.items():
        desc = grpc_api._POOL.FindMessageTypeByName(f"llmss.{name}")
        assert [f.name for f in desc.fields] == [f[0] for f in fields], name
        for f, (fname, num, ftype, rep) in zip(desc.fields, fields):
            assert f.number == num, (name, fname)
            repeated = f.is_repeated if hasattr(f, "is_repeated") else f.label == F.LABEL_REPEATED
            assert repeated == rep, (name, fname)
            if ftype in scalar:
                assert f.type == scalar[ftype], (name, fname)
            else:
                assert f.type == F.TYPE_MESSAGE and f.message_type.name == ftype, (name, fname)
    req = grpc_api._POOL.FindMessageTypeByName("llmss.GenerateRequest")
    assert (req.fields_by_name["return_logprobs"].number, req.fields_by_name["top_logprobs"].number) == (11, 12)
    resp = grpc_api._POOL.FindMessageTypeByName("llmss.GenerateResponse")
    assert (resp.fields_by_name["token_logprobs"].number, resp.fields_by_name["top_logprobs"].number) == (8, 9)
    tokd = grpc_api._POOL.FindMessageTypeByName("llmss.Token")
    assert (tokd.fields_by_name["logprob"].number, tokd.fields_by_name["top"].number) == (5, 6)


def test_server_launch_flag():
    import argparse

    from llmss_amd.serving.launch import add_engine_args

    p = add_engine_args(argparse.ArgumentParser())
    assert p.parse_args([]).max_logprobs == 0
    assert p.parse_args(["--max-logprobs", "5"]).max_logprobs == 5
