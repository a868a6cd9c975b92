"""sirgcn — MI355X-native SIRConv (briangodwinlim/SIR-GCN ``models/conv.py``) hot path.

    import sys; sys.path.insert(0, "<repo>/sir-gcn_amd")
    from sirgcn import SIRConv, Graph      # drop-in for `from models.conv import SIRConv`
"""
from .conv import SIRConv, EdgeAggregate, activation_code  # noqa: F401
from .graph import Graph, GraphPlan, RowCSR, batch, get_plan, build_row_csr  # noqa: F401
from .norm import GraphNorm, GraphBatchNorm, GraphLayerNorm, GetNorm  # noqa: F401
from .econv import SIREConv  # noqa: F401
from .readout import SumPooling, AvgPooling, MaxPooling, readout_nodes, broadcast_nodes  # noqa: F401
from .propagate import label_spreading, correct_and_smooth, Clamp, FixRows  # noqa: F401
from .dropedge import DropEdge, drop_edges, drop_edge_keep  # noqa: F401
from .prenorm import drop_act, PreNormSIRModel  # noqa: F401
from .regularize import param_norms, regularizer  # noqa: F401
from . import _native  # noqa: F401

__all__ = ["param_norms", "regularizer", "drop_act", "PreNormSIRModel", "DropEdge", "drop_edges", "drop_edge_keep", "label_spreading", "correct_and_smooth", "Clamp", "FixRows",
"SIRConv", "SIREConv", "GraphNorm", "GraphBatchNorm", "GraphLayerNorm", "GetNorm", "Graph", "GraphPlan", "RowCSR", "EdgeAggregate", "batch", "get_plan",
           "build_row_csr", "SumPooling", "AvgPooling", "MaxPooling", "readout_nodes", "broadcast_nodes"]
