"""CPU: the emulation of one classification head under classif_dropout (tests/head_dropout_ref.py) against its float64 reference, at the
shapes, seeds and masks the recorded figures name.

The composed-head bounds of test_classif_dropout_ops_gpu.py are 2 x a figure of head_dropout_ref.EMU*; this module re-measures each figure
(printing it: run with -s) and fails when the measurement exceeds the recorded figure, or when the recorded figure has grown slack (more than
1.5 x the measurement), so a bound can neither be missed by the emulation itself nor be widened quietly."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import head_dropout_ref as HD  # noqa: E402
import loss_ref as R  # noqa: E402


def _holds(measured, recorded, what):
    print("%-40s measured %.4e  recorded %.4e" % (what, measured, recorded))
    assert measured <= recorded, (what, measured, recorded)
    assert recorded <= 1.5 * measured, (what, "recorded figure is slack", measured, recorded)


def test_scale_is_the_fp32_value_the_engine_computes():
    one = torch.tensor(1.0, dtype=torch.float32)
    assert HD.THR16 == int(round(HD.P * 65536))
    assert HD.SCALE == float(one / (one - torch.tensor(float(HD.THR16), dtype=torch.float32) / 65536.0))
    assert float(torch.tensor(HD.SCALE, dtype=torch.float32)) == HD.SCALE          # exactly an fp32 value


def test_reference_is_the_reference_heads_forward_under_the_masks():
    """head_ref's forward is dropout(x) -> dense -> tanh -> dropout -> out_proj with the two masks in call order (reference
    src/model/model.py:133-158 builds HF BartClassificationHead(input_dim, inner_dim, num_classes, classif_dropout))"""
    k = HD.case("rel")
    m_in, m_h = HD.bernoulli_masks(k)
    masks = iter((m_in, m_h))

    def dropout(x):
        return x * (R.f64(next(masks)) * HD.SCALE)

    x = torch.cat([R.f64(k["hdec"])[r.long()] for r in k["rows"]], dim=1)
    x = dropout(x)
    x = torch.tanh(F.linear(x, R.f64(k["Wd"]), R.f64(k["bd"])))
    x = dropout(x)
    lg = F.linear(x, R.f64(k["Wo"]), R.f64(k["bo"]))
    ref = HD.head_ref(k, m_in, m_h)
    assert torch.allclose(lg, ref["logits"], rtol=1e-12, atol=1e-14)
    assert torch.allclose(k["factor"] * F.cross_entropy(lg, k["labels"]), ref["loss"], rtol=1e-12)
    # the masks drop about a tenth and the gathered rows repeat: what the bounds below are measured on
    assert abs(float((~m_in).float().mean()) - HD.P) < 0.01 and abs(float((~m_h).float().mean()) - HD.P) < 0.01
    assert len(set(k["rows"][0].tolist())) < k["n"]


@pytest.mark.parametrize("name", ["mrm", "rel"])
def test_head_dropout_emulation(name):
    got = HD.measure(name)
    for q, recorded in HD.EMU[name].items():
        _holds(got[q], recorded, "%s head %s" % (name, q))
    _holds(got["worst_row"], HD.EMU_WORST_ROW[name], "%s head d_states worst row" % name)
    _holds(got["loss"], HD.EMU_LOSS[name], "%s head loss" % name)
    # dropped inputs get no gradient and the head's own gradient dominates the rows it touches
    k = HD.case(name)
    m_in, m_h = HD.bernoulli_masks(k)
    ref = HD.head_ref(k, m_in, m_h)
    t = torch.cat(k["rows"]).long().unique()
    assert float((ref["d_states"][t] - R.f64(k["dhdec"])[t]).norm()) > float(R.f64(k["dhdec"])[t].norm())
