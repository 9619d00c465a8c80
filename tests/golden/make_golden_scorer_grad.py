"""Fixtures of the input gradient of the DeepSpeech2 scorer and of AutoencoderLoss2's recognition term, produced by the
reference's own CPU PyTorch code (phoneme_recognition/deepspeech2.py, phoneme_to_articulation/principal_components/losses.py).
Run from the repository root with the reference checkout at make_golden.REF, after make_golden.py (the scorer cases reuse the
weights and inputs of its deepspeech2_small / deepspeech2_plain fixtures):

    python tests/golden/make_golden_scorer_grad.py

Writes tests/golden/scorer_grad.npz.  Every recognizer is in eval() mode: the reference's loss module never switches it, so
there it runs in training mode with dropout; this engine scores in eval mode."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _load, save, sd_to_np  # noqa: E402
from make_golden_pc_training import ARTS, COMPS, HIDDEN, N, _batch, _normalizers, load_reference  # noqa: E402

SCORER_CASES = ("deepspeech2_small", "deepspeech2_plain")
# the loss's recognizer: 2 coordinate planes of len(ARTS) x N points (30 features), through an adapter to 16
RECOGNIZER = dict(in_channels=2, num_residual_layers=2, num_rnn_layers=1, rnn_hidden_size=32, num_classes=7,
                  num_features=len(ARTS) * N, adapter_out_features=16)


def _frozen(ds2, seed, **kw):
    torch.manual_seed(seed)
    model = ds2.DeepSpeech2(dropout=0.1, **kw)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.7, 1.3)
                m.bias.uniform_(-0.2, 0.2)
    for p in model.parameters():
        p.requires_grad = False
    return model.eval()


def gen_scorer(ds2, arrays, checks):
    """dx of the scorer for a fixed upstream gradient on the features only, the logits only, and both."""
    for name in SCORER_CASES:
        with np.load(os.path.join(OUT, name + ".npz")) as z:
            g = {k: z[k] for k in z.files}
        c = [int(v) for v in g["cfg"]]
        model = ds2.DeepSpeech2(c[0], c[1], c[2], c[3], num_classes=c[4], num_features=c[5], dropout=0.1,
                                adapter_out_features=c[6] or None)
        model.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w.")})
        for p in model.parameters():
            p.requires_grad = False
        model.eval()
        voicing = torch.from_numpy(g["voicing"]) if "voicing" in g else None
        gen = torch.Generator().manual_seed(41)
        gl = torch.randn(g["logits"].shape, generator=gen)
        gf = torch.randn(g["features"].shape, generator=gen)
        for kind in ("feat", "logits", "both"):
            x = torch.from_numpy(g["x"]).clone().requires_grad_(True)
            logits, features = model(x, voicing, return_features=True)
            if kind == "feat":
                features.backward(gf)
            elif kind == "logits":
                logits.backward(gl)
            else:
                torch.autograd.backward([logits, features], [gl, gf])
            arrays[f"{name}.dx_{kind}"] = x.grad.numpy()
            checks[f"{name}.dx_{kind}"] = float(x.grad.double().abs().sum())
        arrays[f"{name}.gl"], arrays[f"{name}.gf"] = gl.numpy(), gf.numpy()


def gen_loss(ds2, ae, losses, transforms, tmp, arrays, checks):
    """AutoencoderLoss2 with a recognizer: beta4 in {0.5, 1}, rescale_factor in {1, 12}, ragged lengths, voicing padded with -1."""
    recognizer = _frozen(ds2, 211, **RECOGNIZER)   # one recognizer for every case
    arrays.update(sd_to_np("rec_model.", recognizer.state_dict()))
    for case, beta4, rescale in (("b05_r1", 0.5, 1.0), ("b1_r1", 1.0, 1.0), ("b05_r12", 0.5, 12.0), ("b1_r12", 1.0, 12.0)):
        seed = {"b05_r1": 111, "b1_r1": 112, "b05_r12": 113, "b1_r12": 114}[case]
        torch.manual_seed(seed)
        enc = ae.MultiEncoder(COMPS, 2 * N, HIDDEN, encoder_cls="AE")
        dec = ae.MultiDecoder(COMPS, 2 * N, HIDDEN, decoder_cls="AE")
        torch.save(enc.state_dict(), os.path.join(tmp, "enc.pt"))
        torch.save(dec.state_dict(), os.path.join(tmp, "dec.pt"))
        g = torch.Generator().manual_seed(seed)
        norm = _normalizers(transforms, g)
        crit = losses.AutoencoderLoss2(COMPS, ["LA", "TTCD"], 2 * N, HIDDEN, os.path.join(tmp, "enc.pt"), os.path.join(tmp, "dec.pt"),
                                       "cpu", encoder_cls="AE", decoder_cls="AE",
                                       denormalize_fn={a: n.inverse for a, n in norm.items()}, beta1=0.7, beta2=1.3, beta3=0.4,
                                       beta4=beta4, rescale_factor=rescale, recognizer=recognizer)
        lengths, targets, ref, mask = _batch(g, 5, 9)
        voicing = (torch.rand(5, 9, generator=g) > 0.5).float()
        for b, l in enumerate(lengths.tolist()):
            voicing[b, l:] = -1.0   # the collate function's padding value
        pcs = ((torch.rand(5, 9, sum(COMPS.values()), generator=g) * 2 - 1) / rescale).requires_grad_(True)
        loss = crit(pcs, targets, ref, lengths, mask, voicing)
        loss.backward()
        p = f"rec_{case}."
        arrays.update(sd_to_np(p + "enc.", enc.state_dict()))
        arrays.update(sd_to_np(p + "dec.", dec.state_dict()))
        arrays.update({p + "pcs": pcs.detach().numpy(), p + "targets": targets.numpy(), p + "ref": ref.numpy(), p + "mask": mask.numpy(),
                       p + "lengths": lengths.numpy(), p + "voicing": voicing.numpy(), p + "loss": np.array(loss.item()),
                       p + "dpcs": pcs.grad.numpy(), p + "rescale": np.array(rescale), p + "betas": np.array([0.7, 1.3, 0.4, beta4])})
        for a in ARTS:
            arrays[p + f"norm_mean.{a}"] = norm[a].mean.numpy()
            arrays[p + f"norm_std.{a}"] = norm[a].std.numpy()
        checks[f"rec_{case}"] = dict(seed=seed, loss=float(loss))
    arrays["rec_cfg"] = np.array(json.dumps(RECOGNIZER))


def main():
    _, _, transforms, ae, losses, _, _, _ = load_reference()
    ds2 = _load("ref_deepspeech2", "phoneme_recognition/deepspeech2.py")
    arrays, checks = {}, {}
    gen_scorer(ds2, arrays, checks)
    with tempfile.TemporaryDirectory() as tmp:
        gen_loss(ds2, ae, losses, transforms, tmp, arrays, checks)
    arrays["checks"] = np.array(json.dumps(checks))
    save("scorer_grad", **arrays)
    print(json.dumps(checks, indent=1))


if __name__ == "__main__":
    main()
