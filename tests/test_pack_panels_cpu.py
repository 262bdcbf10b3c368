"""The reference panel packer (ops/reference.py pack_panels): the layout the packed decode GEMM plans read,
``[ceil(N/16)][ceil(K/64)][16][64]`` with element (n, k) at ``[n // 16, k // 64, n % 16, k % 64]`` and zeros past N
and K. It is the oracle of the device packer (tests/test_packed_gemm_gpu.py) and the CPU path."""
import pytest
import torch

from llmss_amd.ops import reference as R

SHAPES = [(16, 64), (40, 200), (80, 192), (208, 72)]


def _weight(N, K):
    # every element distinct and non-zero, exact in bf16: 1 + index / 2^k would round; use int16 bit patterns instead
    bits = (torch.arange(N * K, dtype=torch.int32) % 0x7F00 + 0x80).to(torch.int16)
    return bits.view(torch.bfloat16).view(N, K)


@pytest.mark.parametrize("N,K", SHAPES)
def test_every_element_lands_where_the_layout_formula_says(N, K):
    w = _weight(N, K)
    p = R.pack_panels(w)
    NP, KP = -(-N // 16), -(-K // 64)
    assert p.shape == (NP, KP, 16, 64) and p.dtype == w.dtype and p.is_contiguous()
    flat = p.reshape(-1).view(torch.int16)
    n, k = torch.meshgrid(torch.arange(N), torch.arange(K), indexing="ij")
    idx = (n // 16) * (KP * 1024) + (k // 64) * 1024 + (n % 16) * 64 + (k % 64)
    assert torch.equal(flat[idx.reshape(-1)], w.view(torch.int16).reshape(-1))
    # everything else is padding, and padding is zero bits
    pad = torch.ones(flat.numel(), dtype=torch.bool)
    pad[idx.reshape(-1)] = False
    assert int(pad.sum()) == NP * KP * 1024 - N * K
    assert not flat[pad].any()


@pytest.mark.parametrize("N,K", SHAPES)
def test_unpack_inverts_pack(N, K):
    w = _weight(N, K)
    back = R.unpack_panels(R.pack_panels(w), N, K)
    assert back.shape == w.shape and torch.equal(back.view(torch.int16), w.view(torch.int16))


def test_strided_source():
    big = _weight(48, 256)
    w = big[3:43, 8:208]  # rows 512 B apart, start not 16-byte aligned to a row
    assert torch.equal(R.pack_panels(w).view(torch.int16), R.pack_panels(w.contiguous()).view(torch.int16))
