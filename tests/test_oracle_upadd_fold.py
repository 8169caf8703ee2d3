"""CPU: the conditions that make a ZERO tolerance legitimate for every case of tests/test_gpu_upadd_fold.py's FOLD_CASES (the up-sample +
skip add folded into the DeformConv that writes its skip; reference: tests/lattice_ref.py `exact_fold`).

  * the producer is a lattice DeformConv as tests/test_oracle_lattice.py pins them: integer offsets that vary per pixel and reach 12,
    binary masks, fp32 contraction = fp64, integer outputs, at most 2 % of them beyond the exactly representable range, ReLU clipping
    between 5 % and 40 %;
  * the sum evaluated in fp32 in upadd_vec's order (acc = 0, valid taps ascending, then + skip) equals the fp64 sum, and every sum is a
    multiple of 1/8;
  * with bf16 output the final rounding changes at least a tenth of the sums of the 24 x 40 maps (the pack is exercised; fp16 holds every
    sum, which is fine: a wrong pack format changes every word);
  * the loop-form restatement equals the reference bit for bit, and each of four defects of the folding tail (row / column phases exchanged
    in the tap index, a clamped border tap, a channel group on group 0's taps, an image on image 0's map) changes at least one output of
    every (image, 64-channel group) it concerns -- and nothing else, for the last two."""
import pytest
import torch

import lattice_ref as L
import test_gpu_upadd_fold as G

LIMIT = 2.0 ** 24
MIN_ROUNDED = 0.1


def _producers():
    return list(dict.fromkeys(c.shape for c in G.FOLD_CASES))


def _sums():
    """One entry per distinct (producer, f, node type, stored type) of the table."""
    return list(dict.fromkeys((c.shape, c.f) + G.MODES[m][3:] for c in G.FOLD_CASES for m in c.modes))


def _id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v).replace("torch.", "")


@pytest.mark.parametrize("shape", _producers(), ids=_id)
def test_fold_producers_have_integer_offsets_binary_masks_and_exact_sums(shape):
    B, Ci, Co, H, W = shape
    x, w, b, wo, bo = L.dcn_operands(*shape)
    om = L.dcn_offsets(x, wo, bo)
    off, mask = om[:, :18], torch.sigmoid(om[:, 18:].float())
    assert torch.equal(off, off.round()) and float(off.abs().max()) == 12.0
    assert float(off.std(dim=(0, 2, 3)).min()) > 0.0
    assert set(off.abs().amax(dim=(0, 2, 3)).tolist()) == {3.0, 6.0, 12.0}
    assert bool(((mask == 0.0) | (mask == 1.0)).all()) and float(mask[:, 4].min()) == 1.0 and float(mask.min()) == 0.0
    pre = L.fold_pre(*shape)
    assert torch.equal(L.dcn_pre(x, w, b, wo, bo, acc_dtype=None), pre)
    assert torch.equal(pre, pre.round()) and 3.0 * 9 * Ci + float(b.abs().max()) < LIMIT
    for d, r in L.EXACT_RANGE.items():
        assert float((pre.abs() > r).double().mean()) <= L.MAX_OUTSIDE, (shape, d)
    assert L.RELU_CLIP[0] <= L.clipped_share(pre) <= L.RELU_CLIP[1], L.clipped_share(pre)


@pytest.mark.parametrize("shape,f,node_t,out_t", _sums(), ids=_id)
def test_fold_sums_are_exact_in_fp32_and_the_restatement_is_the_reference(shape, f, node_t, out_t):
    x_lo, w_up = L.fold_operands(*shape, f)[5:]
    assert torch.equal(x_lo, x_lo.round()) and float(x_lo.abs().max()) <= 3.0 and torch.equal(w_up * 8, (w_up * 8).round())
    pre = L.fold_pre(*shape)
    s64 = L.fold_restated(x_lo, w_up, pre, f, node_t, out_t, rounded=False)
    s32 = L.fold_restated(x_lo, w_up, pre, f, node_t, out_t, rounded=False, acc_dtype=torch.float32)
    assert torch.equal(s32.double(), s64)
    assert torch.equal(s64 / L.FOLD_UNIT, (s64 / L.FOLD_UNIT).round()) and float(s64.abs().max()) / L.FOLD_UNIT < LIMIT
    want = L.exact_fold(x_lo, w_up, pre, f, node_t, out_t)
    assert torch.equal(L.fold_restated(x_lo, w_up, pre, f, node_t, out_t), want)
    if out_t == torch.bfloat16 and shape[3:] == (24, 40):
        assert float((want.double() != s64).double().mean()) >= MIN_ROUNDED
    if out_t == torch.float16:
        assert torch.equal(want.double(), s64)


def _groups(diff):
    """{(image, first channel of a 64-channel group): any output differs}."""
    return {(b, g): bool(diff[b, g:g + 64].any()) for b in range(diff.shape[0]) for g in range(0, diff.shape[1], 64)}


@pytest.mark.parametrize("defect", L.FOLD_DEFECTS)
@pytest.mark.parametrize("shape,f,node_t,out_t", _sums(), ids=_id)
def test_each_defect_of_the_folding_tail_changes_every_group_it_concerns(shape, f, node_t, out_t, defect):
    x_lo, w_up = L.fold_operands(*shape, f)[5:]
    pre = L.fold_pre(*shape)
    want = L.exact_fold(x_lo, w_up, pre, f, node_t, out_t)
    seen = _groups(L.fold_restated(x_lo, w_up, pre, f, node_t, out_t, defect=defect) != want)
    concerned = {"swap_rx_ry": lambda b, g: True, "clamp_border": lambda b, g: True, "group0_taps": lambda b, g: g >= 64,
                 "image0_map": lambda b, g: b > 0}[defect]
    for (b, g), differs in seen.items():
        if concerned(b, g):
            assert differs, "%s hides in image %d, channels %d.." % (defect, b, g)
        else:
            assert not differs, "%s reaches image %d, channels %d.." % (defect, b, g)


def test_every_defect_concerns_some_case():
    shapes = [c.shape for c in G.FOLD_CASES if c.folds]
    assert any(s[2] > 64 for s in shapes) and any(s[0] > 1 for s in shapes) and any(s[2] > 128 for s in shapes) and any(s[0] > 2 for s in shapes)
