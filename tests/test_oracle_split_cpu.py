"""The oracle's two halves (oracle/cotr_oracle.py cotr_encode / cotr_decode) and its K/V helper (decoder_kv), which
tests/test_stages_fp64_gpu.py checks the library's stages against.  CPU only."""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import cotr_oracle

_spec = importlib.util.spec_from_file_location(
    'make_golden', os.path.join(os.path.dirname(__file__), 'golden', 'make_golden.py'))
make_golden = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_golden)


@pytest.mark.parametrize('name', list(make_golden.CASES))
def test_decode_of_encode_is_the_forward_bit_for_bit(name):
    sd, img, qs = make_golden.case_inputs(name)
    taps = {}
    ref = cotr_oracle.cotr_forward(sd, img, qs, taps=taps)
    with torch.no_grad():
        enc = cotr_oracle.cotr_encode(sd, img)
        dec = cotr_oracle.cotr_decode(sd, enc['memory'], enc['pos'], qs)
    assert torch.equal(dec['pred_corrs'], ref)
    assert torch.equal(enc['memory'], taps['enc.5']) and torch.equal(enc['pos'], taps['pos'])
    for stage, last in (('layer1', 'layer1.2'), ('layer2', 'layer2.3'), ('layer3', 'layer3.5')):
        assert torch.equal(enc[stage], taps[last]), stage
    assert torch.equal(enc['layer3'], taps['feat'])
    assert torch.equal(dec['hs'], cotr_oracle._ln(taps['dec.5'], sd, 'transformer.decoder.norm.'))


@pytest.mark.parametrize('name', ['single_b1_q1', 'outside_b1_q96'])
def test_decode_of_encode_is_the_forward_in_fp64(name):
    sd, img, qs = make_golden.case_inputs(name)
    with torch.no_grad():
        enc = cotr_oracle.cotr_encode(sd, img, torch.float64)
        dec = cotr_oracle.cotr_decode(sd, enc['memory'], enc['pos'], qs, torch.float64)
    assert torch.equal(dec['pred_corrs'], cotr_oracle.cotr_forward(sd, img, qs, dtype=torch.float64))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_decoder_kv_holds_the_keys_and_values_multi_head_attention_builds(dtype, monkeypatch):
    """decoder_kv against the k / v that multi_head_attention itself computes for each decoder layer (its 2nd and 3rd
    F.linear), recorded from inside the call; every row and column of the [B*512, 6*2*256] layout."""
    sd, img, qs = make_golden.case_inputs('ragged_b2_q257')
    sd = {k: v.to(dtype) for k, v in sd.items()}
    g = torch.Generator().manual_seed(5)
    memory = torch.randn(512, 2, 256, generator=g, dtype=dtype)         # any memory will do: [L,B,E]
    pos = cotr_oracle.image_position_embedding(2, 16, 32, dtype).flatten(2).permute(2, 0, 1)
    tgt = torch.randn(7, 2, 256, generator=g, dtype=dtype)
    kv = cotr_oracle.decoder_kv(sd, memory, pos)
    assert kv.shape == (2 * 512, 6 * 2 * 256) and kv.dtype == dtype
    linear = F.linear
    for layer in range(6):
        seen = []
        monkeypatch.setattr(cotr_oracle.F, 'linear', lambda *a: seen.append(linear(*a)) or seen[-1])
        cotr_oracle.multi_head_attention(tgt, memory + pos, memory, sd, f'transformer.decoder.layers.{layer}.multihead_attn.', 8)
        monkeypatch.setattr(cotr_oracle.F, 'linear', linear)
        assert len(seen) == 4                                            # q, k, v, out_proj
        k, v = (cotr_oracle.seq_to_rows(t) for t in seen[1:3])
        assert torch.equal(kv[:, layer * 512:layer * 512 + 256], k), layer
        assert torch.equal(kv[:, layer * 512 + 256:(layer + 1) * 512], v), layer
    # row b*512 + token of the layout is pair b's token (another GEMM shape: equal to rounding)
    alone = cotr_oracle.decoder_kv(sd, memory[:, 1:2], pos[:, 1:2])
    assert float((kv[512:] - alone).abs().max()) <= (1e-5 if dtype == torch.float32 else 1e-12) * float(alone.abs().max())


def test_layout_converters():
    x = torch.arange(2 * 3 * 4 * 6, dtype=torch.float32).reshape(2, 3, 4, 6)      # [B,C,H,2W]
    sbs = cotr_oracle.nchw_to_sbs(x)
    assert sbs.shape == (2, 4, 6, 3) and sbs[1, 2, 5, 0] == x[1, 0, 2, 5] and sbs.is_contiguous()
    s = torch.arange(5 * 2 * 3, dtype=torch.float32).reshape(5, 2, 3)             # [L,B,E]
    rows = cotr_oracle.seq_to_rows(s)
    assert rows.shape == (10, 3) and torch.equal(rows[5 + 4], s[4, 1])
