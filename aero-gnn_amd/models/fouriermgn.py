"""models/fouriermgn.py drop-in (reference: models/fouriermgn.py:10-183): a MeshGraphNet whose
node encoder reads [node_attr | Fourier features of its first fourier_features_dim columns].
The feature map and the concatenation are one libaerognn pass (agn_fourier_embed through
aerognn.functions.FourierEmbedFn, rounding contract in DESIGN.md); below it the model is
models/mgn.py's: concat EdgeBlock layers on one receiver-grouped level."""
import torch
from torch import nn

from aerognn.functions import FourierEmbedFn
from aerognn.graph import Level
from models.mlp import MLP
from models.mgnLayer import MeshGraphNetLayer


class FourierMeshGraphNet(nn.Module):
    """MeshGraphNet with Fourier embeddings applied to node features before encoding."""

    def __init__(self, input_node_dim: int, input_edge_dim: int, output_node_dim: int, processor_size: int = 15,
                 activation_fn: str = 'relu', num_hidden_layers_node_processor: int = 1,
                 num_hidden_layers_edge_processor: int = 1, hidden_dim_processor: int = 128,
                 num_hidden_layers_node_encoder: int = 1, hidden_dim_node_encoder: int = 128,
                 num_hidden_layers_edge_encoder: int = 1, hidden_dim_edge_encoder: int = 128,
                 aggregation: str = 'sum', hidden_dim_decoder: int = 128, num_hidden_layers_decoder: int = 1,
                 dropout: float = 0.0, fourier_features_dim: int = 2, fourier_freq_start: int = -3,
                 fourier_freq_length: int = 7):
        super().__init__()
        self.fourier_features_dim = fourier_features_dim
        self.fourier_freq_start = fourier_freq_start
        self.fourier_freq_length = fourier_freq_length
        expanded_node_dim = input_node_dim + 2 * fourier_freq_length * fourier_features_dim  # fouriermgn.py:69-70
        self.node_encoder = MLP(expanded_node_dim, hidden_dim=hidden_dim_node_encoder, output_dim=hidden_dim_processor,
                                num_hidden_layers=num_hidden_layers_node_encoder, activation_fn=activation_fn,
                                dropout=dropout, use_layer_norm=True)
        self.edge_encoder = MLP(input_edge_dim, hidden_dim=hidden_dim_edge_encoder, output_dim=hidden_dim_processor,
                                num_hidden_layers=num_hidden_layers_edge_encoder, activation_fn=activation_fn,
                                dropout=dropout, use_layer_norm=True)
        # no do_concat_trick here (fouriermgn.py:91-101): concat EdgeBlocks; `aggregation` is passed
        # through, so anything but 'add' / 'mean' raises ValueError in the forward as in the reference
        self.layers = nn.ModuleList([
            MeshGraphNetLayer(node_dim=hidden_dim_processor, edge_dim=hidden_dim_processor,
                              hidden_dim=hidden_dim_processor,
                              num_hidden_layers_node_processor=num_hidden_layers_node_processor,
                              num_hidden_layers_edge_processor=num_hidden_layers_edge_processor,
                              activation_fn=activation_fn, use_layer_norm=True, aggregation=aggregation)
            for _ in range(processor_size)])
        self.decoder = MLP(input_dim=hidden_dim_processor, hidden_dim=hidden_dim_decoder, output_dim=output_node_dim,
                           num_hidden_layers=num_hidden_layers_decoder, activation_fn=activation_fn,
                           use_layer_norm=False)

    def _embed(self, x, with_input):
        return FourierEmbedFn.apply(x, self.fourier_features_dim, self.fourier_freq_start, self.fourier_freq_length,
                                    with_input)

    def fourier_embedding(self, pos: torch.Tensor) -> torch.Tensor:
        """[cos(2^i pi x), sin(2^i pi x)] of the first fourier_features_dim columns of pos, i in
        [freq_start, freq_start + freq_length): [num_nodes, 2 * freq_length * fourier_features_dim]."""
        return self._embed(pos, False)

    def forward(self, node_attr: torch.Tensor, edge_attr: torch.Tensor, edge_index: torch.Tensor) -> torch.Tensor:
        level = Level.from_edge_index(edge_index, node_attr.shape[0])
        node_hidden = self.node_encoder(self._embed(node_attr, True))  # [node_attr | emb], no torch.cat
        edge_hidden = self.edge_encoder.forward_rows(edge_attr, level.perm)
        for layer in self.layers:
            node_hidden, edge_hidden = layer.forward_level(node_hidden, edge_hidden, level)
        return self.decoder(node_hidden)
