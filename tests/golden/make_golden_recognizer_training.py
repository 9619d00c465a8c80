"""Fixture of training the DeepSpeech2 recogniser (train_phoneme_recognition.py), produced by the reference's own CPU PyTorch code
(phoneme_recognition/deepspeech2.py) and torch's CTC.  Run from the repository root with the reference checkout at make_golden.REF:

    python tests/golden/make_golden_recognizer_training.py

Writes tests/golden/recognizer_training.npz: a small DeepSpeech2 with adapter and voicing in train() mode with dropout=0.0;
log_softmax -> nn.CTCLoss(zero_infinity=True) over ragged input and target lengths (the reference's loss, phoneme_recognition/
__init__.py:112-120, without the logits noise); the logits, the loss and every parameter gradient; the parameters after three
steps of Adam(weight_decay) + CyclicLR(lr / 25, lr, cycle_momentum=False) stepped per batch (train_phoneme_recognition.py)."""
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import REF, _load, install_shims, save, sd_to_np  # noqa: E402

CONFIG = dict(in_channels=2, num_residual_layers=2, num_rnn_layers=2, rnn_hidden_size=16, num_classes=9, num_features=12,
              adapter_out_features=10, dropout=0.0)
LR, WEIGHT_DECAY = 1e-3, 1e-6


def main():
    install_shims()
    sys.path.insert(0, REF)
    _load("settings", "settings.py")
    pkg = types.ModuleType("phoneme_recognition")
    pkg.__path__ = [os.path.join(REF, "phoneme_recognition")]
    sys.modules["phoneme_recognition"] = pkg
    ds2 = _load("phoneme_recognition.deepspeech2", "phoneme_recognition/deepspeech2.py")
    torch.manual_seed(0)
    model = ds2.DeepSpeech2(**CONFIG)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.7, 1.3)
                m.bias.uniform_(-0.2, 0.2)
    model.train()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(1)
    B, T = 3, 14
    x = torch.randn(B, CONFIG["in_channels"], CONFIG["num_features"], T, generator=g)
    voicing = (torch.rand(B, T, generator=g) > 0.5).float()
    input_lengths = torch.tensor([14, 11, 9])
    target_lengths = torch.tensor([5, 2, 4])
    targets = torch.full((B, 5), -1, dtype=torch.long)
    for b in range(B):
        targets[b, : target_lengths[b]] = torch.randint(1, CONFIG["num_classes"], (int(target_lengths[b]),), generator=g)
    targets[0, 2] = targets[0, 1]   # a repeated label
    criterion = torch.nn.CTCLoss(zero_infinity=True)

    def step():
        outputs = model(x, voicing)
        loss = criterion(model.get_normalized_outputs(outputs, use_log_prob=True).permute(1, 0, 2), targets, input_lengths,
                         target_lengths)
        return outputs, loss

    model.zero_grad()
    logits, loss = step()
    loss.backward()
    grads = {"grad/" + n: p.grad.detach().numpy().copy() for n, p in model.named_parameters()}
    model.load_state_dict(init)
    opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=WEIGHT_DECAY)
    sched = torch.optim.lr_scheduler.CyclicLR(opt, base_lr=LR / 25, max_lr=LR, cycle_momentum=False)
    for _ in range(3):
        opt.zero_grad()
        step()[1].backward()
        opt.step()
        sched.step()
    after = {"after/" + n: p.detach().numpy().copy() for n, p in model.named_parameters()}
    cfg = {k: v for k, v in CONFIG.items()}
    save("recognizer_training", config=np.array(json.dumps(cfg)), x=x.numpy(), voicing=voicing.numpy(), targets=targets.numpy(),
         input_lengths=input_lengths.numpy(), target_lengths=target_lengths.numpy(), logits=logits.detach().numpy(),
         loss=np.array(loss.item()), lr=np.array(LR), weight_decay=np.array(WEIGHT_DECAY), **sd_to_np("param/", init), **grads, **after)


if __name__ == "__main__":
    main()
