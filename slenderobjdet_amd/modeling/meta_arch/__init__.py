from .build import META_ARCH_REGISTRY, build_model
from .fcos import FCOS, FCOSV2, FCOSHead, FCOSTopK
from .retinanet import RetinaNet, RetinaNetHead
from .rotated_retinanet import RotatedRetinaNet
from .reppoints import RepPointsDetector
from .fcos_reppoints import FCOSRepPoints, FCOSRepPointsHead
from .rcnn import GeneralizedRCNN, ProposalNetwork, ProposalVisibleRCNN
from .meta import MEAT_HEADS_REGISTRY, AblationMetaArch, AnchorHead, LRTBHead, LRTBTopkHead, PointSetHead
