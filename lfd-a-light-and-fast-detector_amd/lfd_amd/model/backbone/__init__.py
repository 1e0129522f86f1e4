from .lfd_resnet import *
from .resnet import *
