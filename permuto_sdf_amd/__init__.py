"""MI355X-native (gfx950) implementation of the PermutoSDF rendering/training hot path.

Host side: Python/PyTorch-ROCm (device memory, streams, autograd, torch.distributed) calling hand-written
HIP kernels through the C-ABI library declared in include/psdf.h.  No CPU fallback exists.
"""
from . import _lib
from . import image_eval
from . import render
from . import sdf_fit
from . import nerf_train
from . import nerf_view
from . import box_trace
from . import sdf_slice
from . import mesh_color
from .mesh_color import MeshColorizer, VertexColors
from .box_trace import Box, BoxPlayer, BoxTracedFrame, BoxTracer, render_box_traced
from .sdf_slice import PUBU, IsoStyle, SliceImage, SlicePlane, SlicedFrame, cut_slice_into, render_slice
from .encoding import PermutoEncoding, Coarse2Fine
from .mlp import FusedMLP, LipshitzMLP

__all__ = ["PermutoEncoding", "Coarse2Fine", "FusedMLP", "LipshitzMLP", "image_eval", "render", "sdf_fit", "nerf_train", "nerf_view",
           "box_trace", "Box", "BoxTracer", "BoxPlayer", "BoxTracedFrame", "render_box_traced",
           "sdf_slice", "SlicePlane", "IsoStyle", "PUBU", "SliceImage", "SlicedFrame", "render_slice", "cut_slice_into",
           "mesh_color", "MeshColorizer", "VertexColors"]
