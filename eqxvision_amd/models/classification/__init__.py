from .shufflenetv2 import ShuffleNetV2, shufflenet_v2_x0_5, shufflenet_v2_x1_0, shufflenet_v2_x1_5, shufflenet_v2_x2_0
from .squeezenet import SqueezeNet, squeezenet1_0, squeezenet1_1
from .googlenet import BasicConv2d, GoogLeNet, InceptionAux, _Inception, googlenet
from .densenet import DenseNet, _DenseBlock, _DenseLayer, _Transition, densenet121, densenet161, densenet169, densenet201
