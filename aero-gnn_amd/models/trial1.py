"""models/trial1.py drop-in (reference: models/trial1.py:10-116): MeshGraphNet_v2, a MeshGraphNet whose
node encoder also reads a per-graph mean-pooled global feature and whose message passing has a
projection-free edge update:

    g  = mean_pool(linout(mlp(node_attr)))                 per graph            (trial1.py:44-51)
    x  = node_encoder(cat[node_attr, g broadcast])          e = edge_encoder(edge_attr)  (:99-111)
    e' = e + edge_mlp(e);  x' = x + node_mlp(cat[x, scatter_mean(e', col)])     per layer (:61-73)
    decoder(x)                                                                  (:116)

Names, constructor signatures, module registration order and state_dict keys are the reference's:
every chain is the nn.Sequential build_mlp returns, with its ReLU and Dropout slots, so reference
checkpoints load with strict=True and torch.manual_seed gives the same initial weights. The forward
bodies run in libaerognn: each Sequential is one fused chain (aerognn.functions.MLPFn), the pooling
and the broadcast are poolMGN's GlobalPoolFn / BroadcastRowsFn, a layer is one autograd Function
(MGNv2Fn) on a receiver-grouped Level that the model builds once per forward, and float64 goes
through aerognn/f64.py. Dropout > 0 in training is not implemented (as in models/mlp.py).
"""
import torch
from torch import nn

from aerognn import f64
from aerognn.core import Pack, require_device
from aerognn.functions import (BroadcastRowsFn, ChainSpec, GlobalPoolFn, GraphGroups, MGNv2Fn, MLPFn, V2LayerSpec,
                               from_csc, to_csc)
from aerognn.graph import Level
from aerognn.parts import hidden_of, read as read_parts


def build_mlp(input_dim, hidden_dim, output_dim, num_hidden_layers=2, lay_norm=True, pooling=False, dropout=0.0):
    layers = [nn.Linear(input_dim, hidden_dim), nn.ReLU()]
    for _ in range(num_hidden_layers):
        layers += [nn.Linear(hidden_dim, hidden_dim), nn.ReLU(), nn.Dropout(dropout)]
    layers.append(nn.Linear(hidden_dim, output_dim))
    if lay_norm:
        layers.append(nn.LayerNorm(output_dim))
    return nn.Sequential(*layers)


# --------------------------------------------------------------------------- a Sequential as one chain
def _refuse_dropout(seq):
    if isinstance(seq, nn.Sequential) and any(isinstance(m, nn.Dropout) and m.training and m.p > 0 for m in seq):
        raise NotImplementedError("aerognn fused MLP: dropout > 0 in training is not implemented")


def _chain_spec(seq):
    """The ChainSpec of a build_mlp Sequential (or of one Linear), built once and kept on the module."""
    spec = seq.__dict__.get("_agn_spec")
    if spec is None:
        parts = read_parts(seq)
        spec = ChainSpec.of(parts, hidden_of(parts.lins, parts.lins[0][0].shape[0]), Pack())
        spec.check_hidden()
        seq.__dict__["_agn_spec"] = spec
    return spec


def _run(seq, x, rows=None):
    """seq(x) (or seq(x[rows]), the gather fused into the first layer's loads) as one fused chain."""
    _refuse_dropout(seq)
    require_device(x, rows)
    if x.dtype == torch.float64:
        idx = rows.to(torch.int32).contiguous() if rows is not None else None
        return f64.run_chain(f64.Chain.of(read_parts(seq)), [x], [idx])
    s = _chain_spec(seq)
    s.pack.update(x.dtype, x.device)
    return MLPFn.apply(x, s, torch.is_grad_enabled(), rows, *s.params())


class NodeEncoder(nn.Module):
    def __init__(self, node_input_size, hidden_channels, num_hidden_layers=2):
        super(NodeEncoder, self).__init__()
        self.mlp = build_mlp(node_input_size, hidden_channels, hidden_channels, num_hidden_layers)

    def forward(self, x):
        return _run(self.mlp, x)


class EdgeEncoder(nn.Module):
    def __init__(self, edge_input_size, hidden_channels, num_hidden_layers=2):
        super(EdgeEncoder, self).__init__()
        self.mlp = build_mlp(edge_input_size, hidden_channels, hidden_channels, num_hidden_layers)

    def forward(self, edge_attr):
        return _run(self.mlp, edge_attr)

    def forward_rows(self, edge_attr, rows):
        """self.forward(edge_attr[rows]) without the gathered copy (a level's receiver-grouped order)."""
        return _run(self.mlp, edge_attr, rows)


class GlobalEncoder(torch.nn.Module):
    def __init__(self, in_channels, hidden_channels, num_encoder_layers=2):
        super(GlobalEncoder, self).__init__()
        self.mlp = build_mlp(in_channels, hidden_channels, hidden_channels, num_hidden_layers=num_encoder_layers,
                             lay_norm=False, dropout=0.0)
        self.pool = "mean"  # global_mean_pool (trial1.py:40): GlobalPoolFn's segment mean
        self.linout = torch.nn.Linear(hidden_channels, hidden_channels)

    def forward_groups(self, x, groups):
        # (no activation between the chain's last Linear and linout: two chains)
        return GlobalPoolFn.apply(_run(self.linout, _run(self.mlp, x)), groups, self.pool)

    def forward(self, x, edge_index=None, batch=None):
        require_device(x, batch)
        return self.forward_groups(x, GraphGroups(batch, x.size(0), x.device))  # [graphs, hidden_channels]


class MeshGraphNetLayer_v2(nn.Module):
    def __init__(self, hidden_channels):
        super(MeshGraphNetLayer_v2, self).__init__()
        self.edge_mlp = build_mlp(hidden_channels, hidden_channels, hidden_channels)
        self.node_mlp = build_mlp(2 * hidden_channels, hidden_channels, hidden_channels)
        self._spec = None

    def spec(self):
        if self._spec is None:
            self._spec = V2LayerSpec(*(read_parts(m)[:2] for m in (self.edge_mlp, self.node_mlp)))
        return self._spec

    def forward_level(self, x, e, level):
        """Hot path: edge latents already in the level's receiver-grouped (CSC) order."""
        _refuse_dropout(self.edge_mlp)
        _refuse_dropout(self.node_mlp)
        require_device(x, e)
        if x.dtype == torch.float64:
            e_new = f64.run_chain(f64.Chain.of(read_parts(self.edge_mlp)), [e], resid=e)
            agg = f64.SegSum64Fn.apply(e_new, level.rowptr, level.dst, x.shape[0], True)
            return f64.run_chain(f64.Chain.of(read_parts(self.node_mlp)), [x, agg], resid=x), e_new
        s = self.spec()
        s.pack.update(x.dtype, x.device)
        return MGNv2Fn.apply(x, e, level, s, torch.is_grad_enabled(), *s.params())

    def forward(self, x, edge_index, edge_attr):
        require_device(x, edge_index, edge_attr)
        lv = Level.from_edge_index(edge_index, x.shape[0])
        x, e = self.forward_level(x, to_csc(edge_attr, lv), lv)
        return x, from_csc(e, lv)


class MeshGraphNet_v2(nn.Module):
    def __init__(self, node_input_size, edge_input_size, hidden_channels, out_channels, num_graph_conv_layers,
                 num_encoder_layers=2, num_decoder_layers=2, dropout=0.0):
        super(MeshGraphNet_v2, self).__init__()
        self.node_encoder = NodeEncoder(node_input_size + hidden_channels, hidden_channels,
                                        num_hidden_layers=num_encoder_layers)
        self.edge_encoder = EdgeEncoder(edge_input_size, hidden_channels, num_hidden_layers=num_encoder_layers)
        self.extract_feature = GlobalEncoder(node_input_size, hidden_channels, num_encoder_layers=num_encoder_layers)
        self.layers = nn.ModuleList([MeshGraphNetLayer_v2(hidden_channels) for _ in range(num_graph_conv_layers)])
        self.dropout = nn.Dropout(dropout)  # registered and unused, as in the reference (trial1.py:86)
        self.decoder = build_mlp(input_dim=hidden_channels, hidden_dim=hidden_channels, output_dim=out_channels,
                                 num_hidden_layers=num_decoder_layers - 1, lay_norm=False, dropout=dropout)

    def decode(self, x):
        return _run(self.decoder, x)

    def forward(self, node_attr: torch.Tensor, edge_attr: torch.Tensor, edge_index: torch.Tensor, batch):
        _refuse_dropout(self.decoder)
        require_device(node_attr, edge_attr, edge_index, batch)
        n = node_attr.size(0)
        # the pooled rows go back as repeat_interleave(bincount(batch)) (trial1.py:102: g[batch] only
        # for a non-decreasing batch), which is GraphGroups.bcast; batch None = one graph (:104-106)
        groups = GraphGroups(batch, n, node_attr.device)
        g = BroadcastRowsFn.apply(self.extract_feature.forward_groups(node_attr, groups), groups)
        x = self.node_encoder(torch.cat((node_attr, g), dim=-1))
        level = Level.from_edge_index(edge_index, n)
        e = self.edge_encoder.forward_rows(edge_attr, level.perm)
        for layer in self.layers:
            x, e = layer.forward_level(x, e, level)
        return self.decode(x)
