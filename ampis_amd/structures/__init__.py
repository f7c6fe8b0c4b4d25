from .boxes import Boxes, BoxMode
from .instance_set import InstanceSet, RLEMasks
from .instances import Instances
from .masks import BitMasks, PolygonMasks, RLEBitMasks

__all__ = ["Boxes", "BoxMode", "Instances", "BitMasks", "PolygonMasks", "RLEBitMasks", "InstanceSet", "RLEMasks"]
