"""Drop-in mirror of the reference's ``models/bonenet.py`` (its lines 17-125): ``EdgeConv``, ``GCU``,
``ShapeEncoder``, ``JointEncoder`` and ``PairCls`` with the same constructor and ``forward(data, permute_joints=True)`` signatures,
the returned ``(pre_label, gt_label)`` and the same state_dict keys (RigNet / MoRig bonenet checkpoints load with strict=True);
eval-mode arithmetic on the MI355X-native op layer. ``PairCls`` scores every joint pair of every mesh of a batch for connectivity.

Restructurings (exact up to fp32 rounding):
  * the three feature-only GCUs write column windows of one wide buffer [x_1 | x_2 | x_3]; ``scatter_max`` is the pooled epilogue of
    the last ``mlp_glb`` GEMM;
  * the per-mesh shape and joint features are never repeated per pair (``repeat_interleave``, :110-112): their share of
    ``mix_transform``'s first Linear enters as a per-mesh row bias (``packing.couple_rowbias``), as in ``GCNRig``.
Random draws are the reference's, in its order: the FPS starts of ``sa1`` then ``sa2`` (one ``torch.randint`` per cloud), then, with
``permute_joints``, one ``torch.rand(len(pairs))``.
"""
from __future__ import annotations

import torch
from torch.nn import Dropout, Linear, Sequential

from .. import packing
from ..native import Mat
from ..runtime import get_ops
from . import basic_modules as bm
from .basic_modules import MLP, GlobalSAModule, NativeModule, SAModule, _padded_copy
from .rignet import _num_graphs

__all__ = ["EdgeConv", "GCU", "ShapeEncoder", "JointEncoder", "PairCls"]


class EdgeConv(NativeModule):
    """models/bonenet.py:17-39: the feature-only EdgeConv; its MLP is called ``nn`` here (``nn_pos`` in basic_modules)."""

    def __init__(self, in_channels, out_channels, nn, aggr="max", **kwargs):
        super().__init__()
        assert aggr == "max", "only aggr='max' is used by MoRig"
        self.in_channels, self.out_channels = in_channels, out_channels
        self.nn = nn

    def _pack(self):
        vertex, (edge,) = packing.pack_edge_pair([self.nn])
        return dict(vertex=vertex, edge=edge)

    _forward = bm.EdgeConv._forward


class GCU(bm.GCU):
    """models/bonenet.py:42-56: basic_modules.GCU's wiring around this file's EdgeConv."""

    def __init__(self, in_channels, out_channels, aggr="max"):
        NativeModule.__init__(self)
        half = out_channels // 2
        self.edge_conv_tpl = EdgeConv(in_channels, half, nn=MLP([in_channels * 2, half, half]), aggr=aggr)
        self.edge_conv_geo = EdgeConv(in_channels, half, nn=MLP([in_channels * 2, half, half]), aggr=aggr)
        self.mlp = MLP([out_channels, out_channels])

    def _pack(self):
        vertex, (et, eg) = packing.pack_edge_pair([self.edge_conv_tpl.nn, self.edge_conv_geo.nn])
        return dict(vertex=vertex, et=et, eg=eg, mlp=packing.pack_mlp_layer(self.mlp[0]))


class ShapeEncoder(NativeModule):
    """models/bonenet.py:58-72 and, with ``GLB = (128,)``, models/rootnet.py:16-31: three GCUs (3 -> 64 -> 128 -> 256) on the tpl / geo
    graphs, ``mlp_glb`` on their concatenation, the per-mesh column max."""

    WIDTHS = (64, 128, 256)
    GLB = (256, 64)

    def __init__(self, aggr="max"):
        super().__init__()
        w1, w2, w3 = self.WIDTHS
        self.gcu_1 = GCU(in_channels=3, out_channels=w1, aggr=aggr)
        self.gcu_2 = GCU(in_channels=w1, out_channels=w2, aggr=aggr)
        self.gcu_3 = GCU(in_channels=w2, out_channels=w3, aggr=aggr)
        self.mlp_glb = MLP([w1 + w2 + w3, *self.GLB])

    def _pack(self):
        return [packing.pack_mlp_layer(l) for l in self.mlp_glb]

    def _forward(self, data):
        """-> [n_meshes, glb[-1]]"""
        ops = get_ops()
        pos = _padded_copy(ops, data.pos.float().contiguous())
        dev, n = pos.device, pos.shape[0]
        ng = _num_graphs(data, data.batch)
        layers = self.packed(dev)
        csr_tpl, csr_geo = ops.csr_build(data.tpl_edge_index, n), ops.csr_build(data.geo_edge_index, n)
        w1, w2, w3 = self.WIDTHS
        wide = ops.empty(n, w1 + w2 + w3, dev)
        self.gcu_1.run(ops, Mat.of(pos, 0, 3), csr_tpl, csr_geo, Mat.of(wide, 0, w1))
        self.gcu_2.run(ops, Mat.of(wide, 0, w1), csr_tpl, csr_geo, Mat.of(wide, w1, w2))
        self.gcu_3.run(ops, Mat.of(wide, w1, w2), csr_tpl, csr_geo, Mat.of(wide, w1 + w2, w3))
        h = Mat.of(wide)
        for lay in layers[:-1]:
            o = ops.empty(n, lay.N, dev)
            ops.gemm(h, lay, relu=True, Y=Mat.of(o))
            h = Mat.of(o)
        pooled = ops.empty(ng, layers[-1].N, dev)
        ops.gemm(h, layers[-1], relu=True, seg=ops.make_seg(data.batch, ng, 1), pool=pooled)
        return pooled


class JointEncoder(NativeModule):
    """models/bonenet.py:75-96: two set-abstraction levels over a mesh's joints and a global one -> [n_meshes, 128]."""

    def __init__(self):
        super().__init__()
        self.sa1_module_joints = SAModule(0.999, 0.4, MLP([3, 64, 64, 128]), max_num_neighbors=64)
        self.sa2_module_joints = SAModule(0.33, 0.6, MLP([128 + 3, 128, 128, 256]), max_num_neighbors=64)
        self.sa3_module_joints = GlobalSAModule(MLP([256 + 3, 256, 256, 512, 256, 128]))

    def _pack(self):
        return {}

    def _forward(self, joints, joints_batch):
        sa1 = self.sa1_module_joints._forward(None, joints, joints_batch)
        sa2 = self.sa2_module_joints._forward(*sa1)
        return self.sa3_module_joints._forward(*sa2)[0]


def coupled_head(first: Sequential, n_mesh_cols: int):
    """first = Seq(Linear, ReLU, BN) over [per-mesh columns | per-row columns]: -> (g, main) with g the per-mesh share as a row bias"""
    W = first[0].weight.detach()
    main = packing.pack_linear(W[:, n_mesh_cols:], first[0].bias, first[2])
    return packing.couple_rowbias(packing.pack_linear(W[:, :n_mesh_cols]), main), main


def run_head(ops, pk, mesh_feat: torch.Tensor, rows: torch.Tensor, seg: torch.Tensor) -> torch.Tensor:
    """pk: dict(g, main, rest=[PackedLinear ...], last); mesh_feat [n_meshes, C_mesh]; rows [n, C_row]; seg int32 [n] -> [n, 1]"""
    dev, n = rows.device, rows.shape[0]
    gb = ops.empty(mesh_feat.shape[0], pk["g"].N, dev)
    ops.gemm(Mat.of(mesh_feat), pk["g"], relu=False, Y=Mat.of(gb))
    h = ops.empty(n, pk["main"].N, dev)
    ops.gemm(Mat.of(rows), pk["main"], relu=True, Y=Mat.of(h), rowbias=Mat.of(gb), seg=seg)
    for lay in pk["rest"]:
        o = ops.empty(n, lay.N, dev)
        ops.gemm(Mat.of(h), lay, relu=True, Y=Mat.of(o))
        h = o
    out = ops.empty(n, pk["last"].N, dev)
    ops.gemm(Mat.of(h), pk["last"], relu=False, Y=Mat.of(out))
    return out


class PairCls(NativeModule):
    """models/bonenet.py:99-125."""

    def __init__(self):
        super().__init__()
        self.expand_joint_feature = Sequential(MLP([8, 32, 64, 128, 256]))
        self.shape_encoder = ShapeEncoder()
        self.joint_encoder = JointEncoder()
        self.mix_transform = Sequential(MLP([448, 128, 64]), Dropout(0.7), Linear(64, 1))

    def _pack(self):
        mix = self.mix_transform
        g, main = coupled_head(mix[0][0], 64 + 128)            # [shape 64 | joint 128 | pair 256] (:122)
        return dict(expand=[packing.pack_mlp_layer(l) for l in self.expand_joint_feature[0]], g=g, main=main,
                    rest=[packing.pack_mlp_layer(mix[0][1])], last=packing.pack_linear(mix[2].weight, mix[2].bias))

    def _forward(self, data, permute_joints=True):
        ops = get_ops()
        joints = data.joints.float().contiguous()
        dev = joints.device
        joint_feature = self.joint_encoder._forward(joints, data.joints_batch)
        shape_feature = self.shape_encoder._forward(data)
        pairs = data.pairs.long()
        if permute_joints:
            flip = (torch.rand(len(data.pairs)) >= 0.5).long().to(dev).unsqueeze(1)
            first, second = torch.gather(pairs, 1, flip).squeeze(1), torch.gather(pairs, 1, 1 - flip).squeeze(1)
        else:
            first, second = pairs[:, 0], pairs[:, 1]
        x = torch.cat((joints[first], joints[second], data.pair_attr[:, :-1].float()), dim=1).contiguous()
        pk = self.packed(dev)
        h = Mat.of(x)
        for lay in pk["expand"]:
            o = ops.empty(x.shape[0], lay.N, dev)
            ops.gemm(h, lay, relu=True, Y=Mat.of(o))
            h = Mat.of(o)
        ng = shape_feature.shape[0]
        pre_label = run_head(ops, pk, torch.cat((shape_feature, joint_feature), dim=1).contiguous(), h.base,
                             ops.make_seg(data.pairs_batch, ng, 1))
        return pre_label, data.pair_attr[:, -1].unsqueeze(1)
