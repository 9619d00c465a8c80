"""InputTransform of the principal-components method (reference principal_components/transforms.py:4-19): a frozen module
(every parameter requires_grad = False) with an optional activation on its output."""
import torch.nn as nn


class InputTransform(nn.Module):
    def __init__(self, transform, device, activation=None, **kwargs):
        super().__init__()
        self.transform = transform
        self.transform.to(device)
        self.activation = activation
        for parameter in self.transform.parameters():
            parameter.requires_grad = False

    def forward(self, x):
        output = self.transform(x)
        if self.activation is not None:
            output = self.activation(output)
        return output
