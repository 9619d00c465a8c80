"""Host-side pieces of the CTC beam search (no GPU): the entry points are declared, bound and exported, the sizing call and its
formula, the refusals, the new config against main()'s parameters, the default decoder, and the float64 contract itself against
an enumeration of all alignments."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import yaml

import ctc_beam_fp64 as O
from conftest import ROOT

NEW_SYMBOLS = ["as_ctc_beam_workspace_bytes", "as_ctc_beam_search"]


def test_new_symbols_are_declared_bound_and_exported():
    from artspeech_amd import _lib
    header = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in the header"
        assert name in _lib.PROTOTYPES and hasattr(L, name)
    assert "ctc_beam.hip" in __import__("artspeech_amd.build", fromlist=["SOURCES"]).SOURCES
    from artspeech_amd.phoneme_recognition import BeamResult, ctc_beam_search
    from artspeech_amd.phoneme_recognition.beam_search import ctc_beam_search as same
    assert ctc_beam_search is same and BeamResult.__dataclass_fields__.keys() == {"tokens", "counts", "scores", "num_hyps"}


def _expected_bytes(T, B, beam):
    nodes = beam * T + 1
    table = 64
    while table < 2 * nodes:
        table *= 2
    return B * 4 * (nodes + table)


def test_workspace_size_needs_no_device_and_follows_its_formula():
    from artspeech_amd import _lib
    L = _lib.lib()
    for T, B, C, beam in [(200, 32, 45, 50), (1, 1, 2, 1), (8192, 3, 128, 64), (300, 2, 128, 64), (40, 8, 5, 3)]:
        assert L.as_ctc_beam_workspace_bytes(T, B, C, beam) == _expected_bytes(T, B, beam)
    assert L.as_ctc_beam_workspace_bytes(200, 32, 45, 50) == 32 * 4 * (10001 + 32768)
    for T, B, C, beam in [(8193, 1, 45, 50), (200, 1, 129, 50), (200, 1, 1, 50), (200, 1, 45, 65), (200, 1, 45, 0), (0, 1, 45, 50)]:
        assert L.as_ctc_beam_workspace_bytes(T, B, C, beam) == 0      # outside the supported range


def test_cpu_tensors_and_out_of_range_arguments_are_refused():
    from artspeech_amd.phoneme_recognition import ctc_beam_search
    from artspeech_amd.phoneme_recognition.decoders import BeamSearchCTCDecoder
    em = torch.rand(2, 5, 4).log()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ctc_beam_search(em)
    decoder = BeamSearchCTCDecoder(tokens=["_", "a", "b", "c"], blank_token="_")
    with pytest.raises(RuntimeError, match="no CPU path"):
        decoder(em, [5, 5])
    with pytest.raises(RuntimeError, match="no CPU path"):
        decoder.decode_device(em, [5, 5])

    class OnDevice(torch.Tensor):   # argument checks come before anything touches the device
        is_cuda = True

    def dev(*shape):
        return torch.zeros(*shape).as_subclass(OnDevice)

    for kwargs, limit in [(dict(beam_size=65), "64"), (dict(beam_size=0), "64"), (dict(beam_size_token=5), "4 classes"),
                          (dict(beam_size_token=0), "4 classes"), (dict(nbest=0), "at least 1"), (dict(blank=4), r"\[0, 4\)"),
                          (dict(sil=4), r"\[-1, 4\)"), (dict(beam_threshold=-1.0), "at least 0"), (dict(input="logprobs"), "scores")]:
        with pytest.raises(ValueError, match=limit):
            ctc_beam_search(dev(2, 5, 4), **kwargs)
    with pytest.raises(ValueError, match="128"):
        ctc_beam_search(dev(1, 5, 129))
    with pytest.raises(ValueError, match="128"):
        ctc_beam_search(dev(1, 5, 1))
    with pytest.raises(ValueError, match="8192"):
        ctc_beam_search(dev(1, 8193, 4))
    with pytest.raises(ValueError, match="one entry per utterance"):
        ctc_beam_search(dev(2, 5, 4), lengths=[5])
    with pytest.raises(ValueError, match=r"\(B, T, C\)"):
        ctc_beam_search(dev(5, 4))
    with pytest.raises(TypeError, match="float32"):
        ctc_beam_search(torch.zeros(1, 5, 4, dtype=torch.float64).as_subclass(OnDevice))


def test_decoder_takes_torchaudios_arguments_and_refuses_lexicon_and_lm():
    from artspeech_amd.phoneme_recognition.decoders import BeamSearchCTCDecoder, GreedyCTCDecoder, TopKDecoder  # noqa: F401
    params = inspect.signature(BeamSearchCTCDecoder.__init__).parameters
    assert list(params)[1:] == ["tokens", "blank_token", "sil_token", "unk_word", "lexicon", "lm", "nbest", "beam_size",
                                "beam_size_token", "beam_threshold", "sil_score", "log_add", "input"]
    defaults = {k: p.default for k, p in params.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(sil_token=None, unk_word=None, lexicon=None, lm=None, nbest=1, beam_size=50, beam_size_token=None,
                            beam_threshold=50, sil_score=0, log_add=False, input="probs")
    tokens = ["_", "a", "b", "|"]
    with pytest.raises(NotImplementedError, match="lexicon"):
        BeamSearchCTCDecoder(tokens, "_", lexicon="lexicon.txt")
    with pytest.raises(NotImplementedError, match="lm"):
        BeamSearchCTCDecoder(tokens, "_", lm="lm.bin")
    d = BeamSearchCTCDecoder(tokens, "_", sil_token="|", nbest=4, log_add=True)
    assert d.uses_lengths is True and d.blank_index == 0 and d.sil == 3 and d.nbest == 4 and d.log_add is True
    assert BeamSearchCTCDecoder(tokens, 2, sil_token="<sil>").blank_index == 2
    assert BeamSearchCTCDecoder(tokens, 2, sil_token="<sil>").sil == -1


def test_new_config_parses_and_differs_from_the_greedy_one_by_the_decoder_block():
    import decode_phoneme_recognition as E   # imports cleanly: nothing runs at import
    import test_phoneme_recognition as plain
    with open(os.path.join(ROOT, "configs", "test_recognizer_beam_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(ROOT, "configs", "test_recognizer_synthetic.yaml")) as f:
        greedy = yaml.safe_load(f)
    params = inspect.signature(E.main).parameters
    assert set(cfg) <= set(params), set(cfg) - set(params)
    assert params["decoder"].default is None
    # test_phoneme_recognition.main's parameters, in its order and with its defaults, then `decoder`
    assert list(params.values())[:-1] == list(inspect.signature(plain.main).parameters.values()) and list(params)[-1] == "decoder"
    with pytest.raises(NotImplementedError, match="CTC"):
        E.main(**dict(cfg, loss="CE"))
    assert {k: v for k, v in cfg.items() if k not in ("decoder", "save_dir")} == {k: v for k, v in greedy.items() if k != "save_dir"}
    assert cfg["save_dir"] != greedy["save_dir"]
    assert cfg["decoder"]["name"] == "beam" and cfg["decoder"]["nbest"] > 1
    from artspeech_amd.phoneme_recognition.decoders import BeamSearchCTCDecoder
    built = E.make_decoder(cfg["decoder"], ["_", "a", "b"])
    assert isinstance(built, BeamSearchCTCDecoder) and built.nbest == cfg["decoder"]["nbest"] and built.input == "probs"
    assert built.log_add is cfg["decoder"]["log_add"] and built.beam_size == cfg["decoder"]["beam_size"]


def test_main_without_a_decoder_builds_the_greedy_decoder():
    import decode_phoneme_recognition as E
    from artspeech_amd.phoneme_recognition.decoders import GreedyCTCDecoder
    from artspeech_amd.settings import BLANK
    tokens = [BLANK, "a", "b"]
    for block in (None, {"name": "greedy"}):
        built = E.make_decoder(block, tokens)
        assert type(built) is GreedyCTCDecoder and built.blank_index == 0
    with pytest.raises(ValueError, match="neither"):
        E.make_decoder({"name": "viterbi"}, tokens)
    with pytest.raises(ValueError, match="no parameters"):
        E.make_decoder({"name": "greedy", "nbest": 3}, tokens)


def test_main_without_a_beam_decoder_is_test_phoneme_recognitions_own_main(monkeypatch):
    import decode_phoneme_recognition as E
    import test_phoneme_recognition as plain
    with open(os.path.join(ROOT, "configs", "test_recognizer_synthetic.yaml")) as f:
        cfg = yaml.safe_load(f)
    seen = []
    monkeypatch.setattr(plain, "main", lambda **kwargs: seen.append(kwargs) or "its result")
    assert E.main(**cfg) == "its result" and E.main(**cfg, decoder={"name": "greedy"}) == "its result"
    defaults = {k: p.default for k, p in inspect.signature(E.main).parameters.items() if k != "decoder"}
    assert seen == [dict(defaults, **cfg)] * 2 and "decoder" not in seen[0]
    with pytest.raises(ValueError, match="neither"):
        E.main(**cfg, decoder={"name": "viterbi"})
    assert len(seen) == 2


def test_list_form_of_substitution_counts_honours_a_decoder_of_its_own(monkeypatch):
    """The list branch hands TopKDecoder and GreedyCTCDecoder's work to decode_top1 as before, and any other decoder the padded
    batch with each utterance's rows."""
    import artspeech_amd.phoneme_recognition as R
    from artspeech_amd.phoneme_recognition.decoders import GreedyCTCDecoder, TopKDecoder
    calls = []

    def fake_top1(emissions, lengths=None, blank=-1, return_argmax=False):
        calls.append(("top1", tuple(emissions.shape), [int(v) for v in lengths], blank))
        return torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)

    class Own:
        uses_lengths = True
        blank_index = 0

        def decode_device(self, emissions, lengths=None):
            calls.append(("own", tuple(emissions.shape), [int(v) for v in lengths]))
            return torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)

    monkeypatch.setattr(R, "decode_top1", fake_top1)
    monkeypatch.setattr(R, "align_counts", lambda *a: ("counts", None))
    em = [torch.zeros(4, 3), torch.zeros(2, 3)]
    tg = [torch.tensor([1]), torch.tensor([2, 1])]
    for decoder in (GreedyCTCDecoder(["_", "a", "b"], blank_token="_"), TopKDecoder(["_", "a", "b"], blank_token=0), Own()):
        assert R.substitution_counts(em, tg, [3, 2], [1, 2], decoder, None, 3) == "counts"
    assert calls == [("top1", (2, 4, 3), [3, 2], 0), ("top1", (2, 4, 3), [4, 2], 0), ("own", (2, 4, 3), [3, 2])]


# ---------------------------------------------------------------------------------------------- the contract against brute force
SHAPES = [(T, 3) for T in range(1, 5)] + [(T, 4) for T in range(1, 4)] + [(T, 2) for T in range(1, 7)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_equals_the_enumeration_of_all_alignments(seed):
    """log_add with beam 64, K = C and no threshold loses nothing while the reachable states fit the beam: the ranking and the
    scores are those of all C^T alignments grouped by labelling.  Without log_add the best hypothesis is the arg-max path."""
    rng = np.random.default_rng(seed)
    for T, C in SHAPES:
        blank = int(rng.integers(0, C))
        x = O.peaky_emissions(rng, T, C, blank).astype(np.float64)
        exact = O.brute_force(x, blank, log_add=True)
        got = O.beam_search(x, blank, beam_size=64, beam_size_token=C, beam_threshold=np.inf, log_add=True, nbest=len(exact) + 1)
        assert [p for p, _ in got] == [p for p, _ in exact], (T, C)
        np.testing.assert_allclose([s for _, s in got], [s for _, s in exact], rtol=0, atol=1e-9)
        best = O.beam_search(x, blank, beam_size=64, beam_size_token=C, beam_threshold=np.inf, log_add=False, nbest=1)
        assert best[0][0] == O.collapse(x.argmax(1), blank)
        assert abs(best[0][1] - x.max(1).sum()) < 1e-9 and abs(best[0][1] - O.brute_force(x, blank, log_add=False)[0][1]) < 1e-9


def test_oracle_edge_cases_and_tie_rule():
    assert O.beam_search(np.zeros((0, 3))) == [((), 0.0)]
    x = np.log(np.array([[0.5, 0.3, 0.2], [1.0, 1.0, 1.0], [0.2, 0.5, 0.3]]))
    x[1] = -np.inf
    assert O.beam_search(x, nbest=3) == []                                       # a frame of -inf alone: no hypothesis
    # equal values enter the shortlist in ascending class index: K = 1 on a tied row takes class 0
    assert O.beam_search(np.zeros((2, 3)), blank=2, beam_size_token=1, nbest=2) == [((0,), 0.0)]
    # a prefix that dies and is re-created is one hypothesis, not two
    stats = {}
    rng = np.random.default_rng(5)
    x = O.peaky_emissions(rng, 40, 5)
    out = O.beam_search(x, beam_size=3, nbest=3, log_add=True, stats=stats)
    assert len({p for p, _ in out}) == len(out) == 3 and stats["gap"] >= 0 and stats["max_rel"] > 0
    # sil_score moves the silence class's contributions only
    assert O.beam_search(np.zeros((1, 3)), nbest=1, sil=1, sil_score=1.0) == [((1,), 1.0)]
    assert O.beam_search(np.zeros((1, 2)), nbest=2, sil=1, sil_score=-1.0) == [((), 0.0), ((1,), -1.0)]
    assert np.allclose(O.scores_of([[0.25, 0.75]], "probs"), np.log([[0.25, 0.75]]))
    assert np.allclose(np.exp(O.scores_of([[1.0, 2.0, 0.5]], "logits")).sum(), 1.0)
