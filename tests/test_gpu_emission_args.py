"""The six entry points that take an emissions tensor through phoneme_recognition/emission_args.py, each with one set of values
in three memory layouts: contiguous, the permuted view of the other layout (no copy: the time and batch strides reach the
library in swapped places) and a view whose class stride is 2 (the contiguous copy).  The library reads the same numbers in all
three, so every output is the same byte for byte; a stride in the wrong role reads other numbers."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, C = 2, 3, 4
TARGETS = [[1, 2], [3, -1]]
FRAME_TARGETS = [[1, 2, 0], [3, 3, -100]]
INPUT_LENGTHS, TARGET_LENGTHS = [3, 2], [2, 1]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda", 0)


def layouts(values):
    """values (d0, d1, C) -> the same numbers as a contiguous tensor, a permuted view and a view with class stride 2"""
    wide = torch.zeros(*values.shape[:2], 2 * values.shape[2], device=values.device)
    wide[:, :, ::2] = values
    out = [values.contiguous(), values.permute(1, 0, 2).contiguous().permute(1, 0, 2), wide[:, :, ::2]]
    assert out[0].is_contiguous() and not out[1].is_contiguous() and out[1].stride(2) == 1 and out[2].stride(2) == 2
    assert all(torch.equal(o, values) for o in out)
    return out


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8),
                                                                      b.contiguous().reshape(-1).view(torch.uint8))


def run_ctc_loss(x):
    from artspeech_amd.phoneme_recognition.ctc import ctc_loss
    x = x.detach().requires_grad_()
    loss = ctc_loss(x, torch.tensor(TARGETS), INPUT_LENGTHS, TARGET_LENGTHS, reduction="none", logits=True)
    loss.sum().backward()
    return loss.detach(), x.grad


def run_frame_cross_entropy(x):
    from artspeech_amd.phoneme_recognition.frame_ce import frame_cross_entropy
    x = x.detach().requires_grad_()
    loss = frame_cross_entropy(x, torch.tensor(FRAME_TARGETS), INPUT_LENGTHS, INPUT_LENGTHS, label_smoothing=0.1)
    loss.backward()
    return loss.detach(), x.grad


def run_forced_align(x):
    from artspeech_amd.phoneme_recognition.forced_align import forced_align
    al = forced_align(x, torch.tensor(TARGETS), INPUT_LENGTHS, TARGET_LENGTHS, logits=True)
    return al.score, al.frame_index, al.frame_token, al.frame_filled, al.spans, al.span_score


def run_ctc_beam_search(x):
    from artspeech_amd.phoneme_recognition.beam_search import ctc_beam_search
    r = ctc_beam_search(x, INPUT_LENGTHS, nbest=2, log_add=True, input="logits")
    return r.tokens, r.counts, r.scores, r.num_hyps


def run_decode_top1(x):
    from artspeech_amd.phoneme_recognition.align import decode_top1
    return decode_top1(x, INPUT_LENGTHS, blank=0, return_argmax=True)


def run_frame_auroc_counts(x):
    from artspeech_amd.phoneme_recognition.frame_ce import frame_auroc_counts
    return frame_auroc_counts(x, torch.tensor(FRAME_TARGETS), INPUT_LENGTHS)


@pytest.mark.parametrize("run,time_major", [(run_ctc_loss, True), (run_frame_cross_entropy, True), (run_forced_align, False),
                                            (run_ctc_beam_search, False), (run_decode_top1, False), (run_frame_auroc_counts, False)],
                         ids=lambda v: v.__name__[4:] if callable(v) else "")
def test_three_layouts_of_one_tensor_give_the_same_bytes(dev, run, time_major):
    values = torch.randn(B, T, C, generator=torch.Generator().manual_seed(5)).to(dev)   # every row and column distinct
    if time_major:
        values = values.permute(1, 0, 2).contiguous()
    first, *others = [run(x) for x in layouts(values)]
    assert torch.isfinite(first[0].float()).all()   # a loss, an alignment: nothing is vacuous
    for other in others:
        assert len(other) == len(first)
        for a, b in zip(first, other):
            assert same_bytes(a, b)
