"""satrans_amd: the SATrans scenario-adaptive attention path as MI355X (gfx950) HIP kernels behind the
reference's Python API.  See DESIGN.md and INTEGRATION.md."""
from .inputs import DenseFeat, SparseFeat, VarLenSparseFeat, build_input_features, get_feature_names  # noqa: F401
from .callbacks import History  # noqa: F401
from .basemodel import BaseModel  # noqa: F401
from .satrans import SATrans  # noqa: F401
from .layers import (CIN, FM, AdaSparseHead, AFMHead, AFMLayer, AutoIntHead, BiInteractionPooling, BilinearInteraction,  # noqa: F401
                     CrossNet, DCNHead, DeepFMHead, ESMMHead, FeatureEmbedding, FiBiNETHead, InnerProductLayer, InteractingLayer, LinearModel, MDR_BatchNorm,
                     MetaTransformation, MMoEHead, NFMHead, OutterProductLayer, PartitionedNorm, PLEHead, PNNHead, PointLoss, PrunedDNN, RoutedPointLoss, SelfAttention_Layer, SENETLayer,
                     SharedBottomHead, StarHead, StarTowers, WDLHead, XDeepFMHead)
from .optim import TableAdam  # noqa: F401
from .models import (AFM, DCN, ESMM, MMOE, NFM, PLE, PNN, WDL, AdaSparse, AutoInt, DeepFM, FiBiNET, HeadModel, SharedBottom,  # noqa: F401
                     Star_Net, xDeepFM)

__all__ = ["SATrans", "BaseModel", "SparseFeat", "DenseFeat", "VarLenSparseFeat", "get_feature_names",
           "build_input_features", "History", "SelfAttention_Layer", "MetaTransformation",
           "MDR_BatchNorm", "PartitionedNorm", "StarTowers", "StarHead", "MMoEHead", "PLEHead", "PrunedDNN", "AdaSparseHead",
           "SharedBottomHead", "CIN", "XDeepFMHead", "CrossNet", "DCNHead", "SENETLayer", "BilinearInteraction", "FiBiNETHead",
           "InnerProductLayer", "OutterProductLayer", "PNNHead", "FM", "BiInteractionPooling", "AFMLayer", "DeepFMHead", "NFMHead",
           "AFMHead", "InteractingLayer", "AutoIntHead", "ESMMHead", "WDLHead", "LinearModel", "FeatureEmbedding", "TableAdam", "PointLoss", "RoutedPointLoss",
           "HeadModel", "WDL", "DeepFM", "DCN", "MMOE", "Star_Net", "xDeepFM", "NFM", "AFM",
           "AutoInt", "FiBiNET", "PNN", "AdaSparse", "SharedBottom", "PLE", "ESMM"]
