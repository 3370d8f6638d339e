"""ViewEmbeddingMLP (networks/embedding.py:35-62) as a plain nn.Module of PyTorch ops, evaluated per ray: what a caller handed to the blur
kernel modules as `view_embed` before the table kernels existed (they treat a module of any other type than blurmodel's own as per-ray
PyTorch in front of the library).  tools/bench_view_embed.py times this route against the table route."""
import torch
from torch import nn
import torch.nn.functional as F


class TorchViewEmbeddingMLP(nn.Module):
    def __init__(self, D, W, skips, num_embed, embed_dim):
        super().__init__()
        self.skips, self.out_channels, self.embed_dim = skips, W, embed_dim
        self.img_embed = nn.Parameter(torch.zeros(num_embed, embed_dim))
        self.view_embed_linears = nn.ModuleList([nn.Linear(embed_dim, W)] + [nn.Linear(W + embed_dim if i in skips else W, W) for i in range(D - 1)])

    def forward(self, x):
        e = self.img_embed[x]
        h = e
        for i, lin in enumerate(self.view_embed_linears):
            h = F.relu(lin(h))
            if i in self.skips:
                h = torch.cat([e, h], -1)
        return h
