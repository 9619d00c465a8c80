"""Fixtures of the principal-components training path, produced by the reference's own CPU PyTorch code
(phoneme_to_articulation/principal_components/{models/autoencoder,losses,transforms,metrics,dataset,__init__}.py and the two
training scripts' signatures).  Run from the repository root with the reference checkout at make_golden.REF:

    python tests/golden/make_golden_pc_training.py

Writes tests/golden/pc_training.npz: seeds and scalar checks live inside the file (checksums.json is not touched).
Uses make_golden.py's name-only shims for the reference's absent third-party packages."""
import ast
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, _load, _shim, install_shims, save, sd_to_np  # noqa: E402

ARTS = ["lower-lip", "tongue", "upper-lip"]   # sorted; the upper incisor is injected from the reference contour
N = 10                                         # points per contour: in_features = 20
HIDDEN = 10                                    # hidden 10 -> 5: widths that are not multiples of 4
COMPS = {"tongue": 4, "lower-lip": 3, "upper-lip": 2}


def load_reference():
    install_shims()
    sys.path.insert(0, REF)
    settings = _load("settings", "settings.py")
    _load("helpers", "helpers.py")
    pkg = types.ModuleType("phoneme_to_articulation")
    pkg.__path__ = [os.path.join(REF, "phoneme_to_articulation")]
    pkg.InputLoaderMixin = object
    sys.modules["phoneme_to_articulation"] = pkg
    p2a_metrics = _load("phoneme_to_articulation.metrics", "phoneme_to_articulation/metrics.py")
    transforms = _load("phoneme_to_articulation.transforms", "phoneme_to_articulation/transforms.py")
    pc = types.ModuleType("phoneme_to_articulation.principal_components")
    pc.__path__ = [os.path.join(REF, "phoneme_to_articulation/principal_components")]
    sys.modules[pc.__name__] = pc
    models_pkg = types.ModuleType("phoneme_to_articulation.principal_components.models")
    models_pkg.__path__ = [os.path.join(REF, "phoneme_to_articulation/principal_components/models")]
    sys.modules[models_pkg.__name__] = models_pkg
    ae = _load("phoneme_to_articulation.principal_components.models.autoencoder",
               "phoneme_to_articulation/principal_components/models/autoencoder.py")
    for name in ("Encoder", "Decoder", "MultiEncoder", "MultiDecoder", "MultiArticulatorAutoencoder", "EncoderType",
                 "DecoderType", "PCAEncoder", "PCADecoder"):
        setattr(models_pkg, name, getattr(ae, name))
    _load("phoneme_to_articulation.principal_components.transforms", "phoneme_to_articulation/principal_components/transforms.py")
    losses = _load("phoneme_to_articulation.principal_components.losses", "phoneme_to_articulation/principal_components/losses.py")
    metrics = _load("phoneme_to_articulation.principal_components.metrics",
                    "phoneme_to_articulation/principal_components/metrics.py")
    _shim("database_collector", DATABASE_COLLECTORS={})
    dataset = _load("ref_pc_dataset", "phoneme_to_articulation/principal_components/dataset.py")
    loop = _load("ref_pc_init", "phoneme_to_articulation/principal_components/__init__.py")
    return settings, p2a_metrics, transforms, ae, losses, metrics, dataset, loop


def _signature(relpath):
    """main()'s keyword names and defaults, and the argparse flags (option, dest, default) of a reference training script."""
    tree = ast.parse(open(os.path.join(REF, relpath)).read())
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    names = [a.arg for a in main.args.args]
    defaults = [ast.literal_eval(d) for d in main.args.defaults]
    keys = {n: None for n in names}
    keys.update(dict(zip(names[len(names) - len(defaults):], defaults)))
    flags = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument":
            kw = {k.arg: ast.literal_eval(k.value) for k in node.keywords}
            flags.append([node.args[0].value, kw.get("dest"), kw.get("default")])
    return {"main": [[n, keys[n]] for n in names], "flags": flags}


def _normalizers(transforms, g):
    return {a: transforms.Normalize(torch.rand(2, N, generator=g) * 0.2, 0.5 + torch.rand(2, N, generator=g)) for a in ARTS}


def _batch(g, B, T):
    lengths = torch.tensor(sorted([T, 1] + torch.randint(1, T + 1, (B - 2,), generator=g).tolist(), reverse=True))
    targets = torch.rand(B, T, len(ARTS), 2, N, generator=g)
    ref = torch.rand(B, T, 1, 2, N, generator=g)
    mask = (torch.rand(B, 2, T, generator=g) > 0.5).int()
    for b, l in enumerate(lengths.tolist()):
        targets[b, l:] = 0
        mask[b, :, l:] = 0
    return lengths, targets, ref, mask


def gen_autoencoder_loss2(ae, losses, transforms, tmp, arrays, checks):
    for case, kind, rescale in (("ae_r1", "AE", 1.0), ("ae_r12", "AE", 12.0), ("pca", "PCA", 1.0)):
        seed = {"ae_r1": 61, "ae_r12": 62, "pca": 63}[case]
        torch.manual_seed(seed)
        enc = ae.MultiEncoder(COMPS, 2 * N, HIDDEN, encoder_cls=kind)
        dec = ae.MultiDecoder(COMPS, 2 * N, HIDDEN, decoder_cls=kind)
        if kind == "PCA":   # an SVD-built projection, like the scikit-learn PCA of the reference
            data = torch.randn(200, 2 * N, dtype=torch.float64)
            _, S, Vh = torch.linalg.svd(data - data.mean(0), full_matrices=False)
            with torch.no_grad():
                for a, n in COMPS.items():
                    enc.encoders[a].eigenvectors.copy_(Vh[:n].float())
                    enc.encoders[a].eigenvalues.copy_((S[:n] ** 2 / 199).float())
                    dec.decoders[a].eigenvectors.copy_(Vh[:n].float())
        torch.save(enc.state_dict(), os.path.join(tmp, "enc.pt"))
        torch.save(dec.state_dict(), os.path.join(tmp, "dec.pt"))
        g = torch.Generator().manual_seed(seed)
        norm = _normalizers(transforms, g)
        crit = losses.AutoencoderLoss2(COMPS, ["LA", "TTCD"], 2 * N, HIDDEN, os.path.join(tmp, "enc.pt"), os.path.join(tmp, "dec.pt"),
                                       "cpu", encoder_cls=kind, decoder_cls=kind,
                                       denormalize_fn={a: n.inverse for a, n in norm.items()}, beta1=0.7, beta2=1.3, beta3=0.4,
                                       rescale_factor=rescale)
        lengths, targets, ref, mask = _batch(g, 5, 9)
        pcs = ((torch.rand(5, 9, sum(COMPS.values()), generator=g) * 2 - 1) / rescale).requires_grad_(True)
        loss = crit(pcs, targets, ref, lengths, mask)
        loss.backward()
        p = f"ael2_{case}."
        arrays.update(sd_to_np(p + "enc.", enc.state_dict()))
        arrays.update(sd_to_np(p + "dec.", dec.state_dict()))
        arrays.update({p + "pcs": pcs.detach().numpy(), p + "targets": targets.numpy(), p + "ref": ref.numpy(), p + "mask": mask.numpy(),
                       p + "lengths": lengths.numpy(), p + "loss": np.array(loss.item()), p + "dpcs": pcs.grad.numpy(),
                       p + "rescale": np.array(rescale), p + "betas": np.array([0.7, 1.3, 0.4])})
        for a in ARTS:
            arrays[p + f"norm_mean.{a}"] = norm[a].mean.numpy()
            arrays[p + f"norm_std.{a}"] = norm[a].std.numpy()
        checks[f"ael2_{case}"] = dict(seed=seed, kind=kind, loss=float(loss))


def gen_regularized(ae, losses, arrays, checks):
    torch.manual_seed(71)
    model = ae.MultiArticulatorAutoencoder(in_features=2 * N, indices_dict=COMPS, hidden_features=HIDDEN)
    crit = losses.RegularizedLatentsMSELoss2(alpha=0.3, indices_dict=model.indices_dict)
    x = torch.rand(37, len(ARTS), 2 * N)
    w = torch.rand(37)
    out, latent = model(x)
    loss = crit(out, latent, x, w)
    loss.backward()
    arrays.update(sd_to_np("rl.w.", model.state_dict()))
    arrays.update({"rl.g." + k: p.grad.numpy() for k, p in model.named_parameters()})
    arrays.update({"rl.x": x.numpy(), "rl.weights": w.numpy(), "rl.loss": np.array(loss.item()), "rl.alpha": np.array(0.3)})
    checks["rl"] = dict(seed=71, loss=float(loss))


def gen_p2cp(ae, metrics, transforms, settings, tmp, arrays, checks):
    torch.manual_seed(81)
    dec = ae.MultiDecoder(COMPS, 2 * N, HIDDEN)
    torch.save(dec.state_dict(), os.path.join(tmp, "dec.pt"))
    g = torch.Generator().manual_seed(81)
    norm = _normalizers(transforms, g)
    metric = metrics.DecoderMeanP2CPDistance2(settings.DATASET_CONFIG["artspeech2"], os.path.join(tmp, "dec.pt"), COMPS,
                                              {"in_features": 2 * N, "hidden_features": HIDDEN},
                                              {a: n.inverse for a, n in norm.items()}, "cpu")
    lengths, targets, _, _ = _batch(g, 4, 7)
    outputs = torch.rand(4, 7, sum(COMPS.values()), generator=g) * 2 - 1
    targets_in = targets.clone()
    with torch.no_grad():
        value = metric(outputs, targets, lengths)
    arrays.update(sd_to_np("p2cp.dec.", dec.state_dict()))
    arrays.update({"p2cp.outputs": outputs.numpy(), "p2cp.targets_in": targets_in.numpy(), "p2cp.targets_after": targets.numpy(),
                   "p2cp.lengths": lengths.numpy(), "p2cp.value": np.array(value.item())})
    for a in ARTS:
        arrays[f"p2cp.norm_mean.{a}"] = norm[a].mean.numpy()
        arrays[f"p2cp.norm_std.{a}"] = norm[a].std.numpy()
    checks["p2cp"] = dict(seed=81, value=float(value))


def gen_collate(dataset, arrays, checks):
    g = torch.Generator().manual_seed(91)
    items = []
    for i, T in enumerate((4, 7, 2, 7)):
        tokens = torch.randint(2, 30, (T,), generator=g)
        items.append((f"s{i}", tokens, torch.rand(T, 2, 2, 3, generator=g), [f"p{int(t)}" for t in tokens],
                      (torch.rand(2, T, generator=g) > 0.5).int(), torch.rand(T, 1, 2, 3, generator=g), [f"{k:04d}" for k in range(T)],
                      (torch.rand(T, generator=g) > 0.5).float()))
    out = dataset.pad_sequence_collate_fn(items)
    for i, it in enumerate(items):
        arrays.update({f"col.in{i}.tokens": it[1].numpy(), f"col.in{i}.targets": it[2].numpy(), f"col.in{i}.mask": it[4].numpy(),
                       f"col.in{i}.ref": it[5].numpy(), f"col.in{i}.voicing": it[7].numpy()})
    arrays.update({"col.ids": np.array(out[0]), "col.tokens": out[1].numpy(), "col.targets": out[2].numpy(), "col.lengths": out[3].numpy(),
                   "col.phonemes": np.array(json.dumps(out[4])), "col.mask": out[5].numpy(), "col.ref": out[6].numpy(),
                   "col.frames": np.array(json.dumps(out[7])), "col.voicing": out[8].numpy()})
    checks["collate"] = dict(seed=91, n_items=len(items))


def gen_autoencoder_loop(ae, losses, loop, arrays, checks):
    torch.manual_seed(101)
    model = ae.MultiArticulatorAutoencoder(in_features=2 * N, indices_dict=COMPS, hidden_features=HIDDEN)
    # copies: state_dict().numpy() shares the parameters' memory, which the Adam steps below update in place
    arrays.update({k: v.copy() for k, v in sd_to_np("loop.w0.", model.state_dict()).items()})
    crit = losses.RegularizedLatentsMSELoss2(alpha=0.1, indices_dict=model.indices_dict)
    step_losses = []

    def criterion(*args):
        value = crit(*args)
        step_losses.append(value.item())
        return value

    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-6)
    g = torch.Generator().manual_seed(101)
    batches = [([f"f{i}"] * 16, torch.rand(16, len(ARTS), 2 * N, generator=g), torch.rand(16, generator=g), ["a"] * 16)
               for i in range(3)]
    info = loop.run_autoencoder_epoch("train", 1, model, batches, opt, criterion, device=torch.device("cpu"))
    for i, b in enumerate(batches):
        arrays[f"loop.x{i}"], arrays[f"loop.weights{i}"] = b[1].numpy(), b[2].numpy()
    arrays.update(sd_to_np("loop.w3.", model.state_dict()))
    arrays.update({"loop.losses": np.array(step_losses), "loop.info_loss": np.array(info["loss"])})
    checks["loop"] = dict(seed=101, losses=step_losses)


def main():
    settings, _, transforms, ae, losses, metrics, dataset, loop = load_reference()
    arrays, checks = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        gen_autoencoder_loss2(ae, losses, transforms, tmp, arrays, checks)
        gen_regularized(ae, losses, arrays, checks)
        gen_p2cp(ae, metrics, transforms, settings, tmp, arrays, checks)
    gen_collate(dataset, arrays, checks)
    gen_autoencoder_loop(ae, losses, loop, arrays, checks)
    sigs = {"autoencoder": _signature("train_principal_components_autoencoder.py"),
            "method": _signature("train_phoneme_to_principal_components.py")}
    arrays["signatures"] = np.array(json.dumps(sigs))
    arrays["checks"] = np.array(json.dumps(checks))
    save("pc_training", **arrays)
    print(json.dumps(checks, indent=1))


if __name__ == "__main__":
    main()
