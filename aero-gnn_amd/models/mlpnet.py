"""models/mlpnet.py drop-in (reference: models/mlpnet.py:8-42): two MLPs with LayerNorm applied
per node, each one fused libaerognn chain (models/mlp.py). The decoder's LayerNorm runs over the
narrow output_node_dim, which the general MLP kernel handles with masked columns."""
from torch import nn

from models.mlp import MLP


class MLPNet(nn.Module):
    """Multi-Layer Perceptron Network for node-level predictions."""

    def __init__(self, input_node_dim: int, output_node_dim: int, hidden_dim: int = 128,
                 num_hidden_layers_encoder: int = 2, num_hidden_layers_decoder: int = 2,
                 activation_fn: str = 'relu', dropout: float = 0.0):
        super().__init__()
        self.mlp = MLP(input_dim=input_node_dim, hidden_dim=hidden_dim, output_dim=hidden_dim,
                       num_hidden_layers=num_hidden_layers_encoder, activation_fn=activation_fn, dropout=dropout,
                       use_layer_norm=True)
        self.decoder = MLP(input_dim=hidden_dim, hidden_dim=hidden_dim, output_dim=output_node_dim,
                           num_hidden_layers=num_hidden_layers_decoder, activation_fn=activation_fn, dropout=dropout,
                           use_layer_norm=True)

    def forward(self, node_attr):
        return self.decoder(self.mlp(node_attr))
