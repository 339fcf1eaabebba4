"""Drop-in mirror of the reference's ``models/rootnet.py`` (its lines 16-93): ``ShapeEncoder``, ``JointEncoder``
and ``ROOTNET`` with the same ``forward(data, shuffle=True)`` signature, the returned ``(x_joint, joints_label)`` and the same
state_dict keys (RigNet / MoRig rootnet checkpoints load with strict=True); eval-mode arithmetic on the MI355X-native op layer.
``ROOTNET`` scores every joint of every mesh of a batch for being the skeleton's root.

The shape encoder is bonenet's with a one-layer ``mlp_glb``; its pooled vector is never repeated per joint (:89): its share of
``back_layers``' first Linear enters as a per-mesh row bias. Random draws are the reference's, in its order: with ``shuffle`` one
``torch.randperm`` per mesh, then the FPS starts of ``sa1`` and of ``sa2`` (one ``torch.randint`` per cloud each).
"""
from __future__ import annotations

import torch
from torch.nn import Linear, Sequential

from .. import packing
from ..runtime import get_ops
from . import bonenet
from .basic_modules import MLP, FPModule, GlobalSAModule, NativeModule, SAModule
from .bonenet import GCU, coupled_head, run_head  # noqa: F401  (the reference imports GCU from bonenet, :12)

__all__ = ["ROOTNET"]


class ShapeEncoder(bonenet.ShapeEncoder):
    """models/rootnet.py:16-31"""

    GLB = (128,)


class JointEncoder(NativeModule):
    """models/rootnet.py:34-61: PointNet++ over a mesh's joints with |x| as the input feature, down two levels to a global vector and
    back up by k-NN interpolation -> [n_joints, 128]."""

    def __init__(self):
        super().__init__()
        self.sa1_joint = SAModule(0.999, 0.4, MLP([4, 64, 64, 128]), max_num_neighbors=64)
        self.sa2_joint = SAModule(0.33, 0.6, MLP([128 + 3, 128, 128, 256]), max_num_neighbors=64)
        self.sa3_joint = GlobalSAModule(MLP([256 + 3, 256, 256, 512]))
        self.fp3_joint = FPModule(1, MLP([512 + 256, 256, 256]))
        self.fp2_joint = FPModule(3, MLP([256 + 128, 128, 128]))
        self.fp1_joint = FPModule(3, MLP([128 + 1, 128, 128]))

    def _pack(self):
        return {}

    def _forward(self, x, pos, batch):
        sa0 = (x, pos, batch)
        sa1 = self.sa1_joint._forward(*sa0)
        sa2 = self.sa2_joint._forward(*sa1)
        sa3 = self.sa3_joint._forward(*sa2)
        fp3 = self.fp3_joint._forward(*sa3, *sa2)
        fp2 = self.fp2_joint._forward(*fp3, *sa1)
        return self.fp1_joint._forward(*fp2, *sa0)[0]


class ROOTNET(NativeModule):
    """models/rootnet.py:64-93."""

    def __init__(self):
        super().__init__()
        self.shape_encoder = ShapeEncoder()
        self.joint_encoder = JointEncoder()
        self.back_layers = Sequential(MLP([128 + 128, 200, 64]), Linear(64, 1))

    def _pack(self):
        back = self.back_layers
        g, main = coupled_head(back[0][0], 128)                # [shape 128 | joint 128] (:91)
        return dict(g=g, main=main, rest=[packing.pack_mlp_layer(back[0][1])], last=packing.pack_linear(back[1].weight, back[1].bias))

    def _forward(self, data, shuffle=True):
        ops = get_ops()
        joints = data.joints.float()
        dev = joints.device
        counts = torch.bincount(data.joints_batch).tolist()
        order, labels, off = [], [], 0
        for c in counts:                                       # :74-86; label 1 marks each mesh's first joint
            lab = torch.zeros(c, 1)
            lab[0, 0] = 1
            idx = torch.randperm(c) if shuffle else torch.arange(c)
            order.append(idx + off)
            labels.append(lab[idx])
            off += c
        joints = joints[torch.cat(order).to(dev)].contiguous()
        x_glb_shape = self.shape_encoder._forward(data)
        joint_feature = self.joint_encoder._forward(torch.abs(joints[:, 0:1]).contiguous(), joints, data.joints_batch)
        x_joint = run_head(ops, self.packed(dev), x_glb_shape, joint_feature, ops.make_seg(data.joints_batch, x_glb_shape.shape[0], 1))
        return x_joint, torch.cat(labels).to(device=dev, dtype=joints.dtype)
