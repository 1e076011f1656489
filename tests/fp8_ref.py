"""Reference quantiser of the FP8 (e4m3) decoder weights, in torch on the CPU.

A weight [N, K] in bf16 becomes one OCP e4m3fn code per element and one power-of-two exponent per row:

  amax_n = max over the FINITE elements of row n of |W[n, k]|
  e_n    = the smallest integer with amax_n * 2^-e_n <= 448, from the exponent and mantissa bits (no log2);
           0 for a row without a finite non-zero element; clamped to [E_MIN, E_MAX]
  code   = round-to-nearest-even(clamp(W[n, k] * 2^-e_n, -448, 448)) into e4m3fn, subnormal codes kept;
           +-inf saturate to +-448 through the clamp, a NaN becomes the NaN code 0x7f | sign

The clamp of the scaled value only acts where e_n was clamped at E_MAX (amax_n above 448 * 2^119) or the element is infinite;
a row clamped at E_MIN keeps its exponent -120 and loses its smallest elements to the subnormal codes and to zero.
E_MAX = 119 keeps 448 * 2^e_n finite in bf16, E_MIN = -120 keeps 2^e_n and 2^-e_n normal floats."""
import torch

E_MIN, E_MAX = -120, 119
FP8_MAX = 448.0


def _pow2(e):
    """2^e as float32, from the exponent field (e int tensor in [-126, 127])"""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def row_exponents(W):
    """int8 [N]: the row exponents of a bf16 matrix, integer arithmetic on the bf16 bits"""
    assert W.dtype == torch.bfloat16 and W.dim() == 2
    mag = W.contiguous().view(torch.int16).to(torch.int32) & 0x7FFF
    mag = torch.where((mag >> 7) == 0xFF, torch.zeros_like(mag), mag)      # inf / NaN do not set the range
    amax = mag.max(dim=1).values                                             # bf16 magnitudes order as their bits do
    ex, man = amax >> 7, amax & 0x7F
    # amax = (1 + man / 128) * 2^(ex - 127) <= 1.75 * 2^(8 + e)  <=>  e >= ex - 135 (+ 1 when man / 128 > 0.75)
    e = ex - 135 + (man > 0x60).to(torch.int32)
    e = torch.where(ex == 0, torch.full_like(e, E_MIN), e)                   # a subnormal amax lies far below 448 * 2^E_MIN
    e = e.clamp(E_MIN, E_MAX)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    return e.to(torch.int8)


def quantize(W):
    """bf16 [N, K] -> (codes uint8 [N, K], exps int8 [N])"""
    exps = row_exponents(W)
    scaled = W.float() * _pow2(-exps.to(torch.int32))[:, None]               # exact: a power of two, no underflow (E_MIN)
    scaled = scaled.clamp(-FP8_MAX, FP8_MAX)                                 # NaN stays NaN
    codes = scaled.to(torch.float8_e4m3fn).view(torch.uint8)
    # a NaN's sign does not survive host arithmetic reliably: its code is written from the weight's own sign bit
    bits = W.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    nan_code = (0x7F | ((bits >> 15) << 7)).to(torch.uint8)
    codes = torch.where(torch.isnan(W), nan_code, codes)
    return codes, exps


def dequantize(codes, exps):
    """(codes uint8 [N, K], exps int8 [N]) -> bf16 [N, K]; exact (3 mantissa bits against 7, 448 * 2^E_MAX is finite)"""
    f = codes.view(torch.float8_e4m3fn).float() * _pow2(exps.to(torch.int32))[:, None]
    out = f.to(torch.bfloat16)
    fin = torch.isfinite(f)
    assert torch.equal(out.float()[fin], f[fin]), "a dequantised value is not a bf16 number"
    return out


def fragment_order(codes):
    """codes [N, K] -> uint8 [N * K] in the order the decode blocks read them: one KiB per (16-row tile n, 64-deep chunk c),
    lane l's 16 bytes at l * 16 = W[n * 16 + (l & 15)][c * 64 + (l >> 4) * 16 .. + 15]"""
    N, K = codes.shape
    assert N % 16 == 0 and K % 64 == 0
    # [n, r, c, g, j] -> [n, c, g, r, j]   (lane = g * 16 + r)
    return codes.view(N // 16, 16, K // 64, 4, 16).permute(0, 2, 3, 1, 4).contiguous().view(-1)


def quantize_model_state(sd, decoder_layers):
    """A copy of state dict `sd` whose six per-layer decoder matrices (q | k | v of the self-attention, its output projection, the
    cross-attention's q and output projection, fc1, fc2) are replaced by dequantize(quantize(bf16(W))): the model M' whose bf16
    decode the FP8 decode of M must reproduce bit for bit.  Rows are quantised one by one, so quantising q, k, v separately equals
    quantising the engine's stacked [q | k | v] matrix."""
    out = dict(sd)
    for l in range(decoder_layers):
        p = "model.decoder.layers.%d." % l
        for n in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "encoder_attn.q_proj",
                  "encoder_attn.out_proj", "fc1", "fc2"):
            k = p + n + ".weight"
            out[k] = dequantize(*quantize(sd[k].to(torch.bfloat16))).float()
    return out
