from colddiff.decolor import DecolorTrainer as Trainer
from colddiff.decolor import DeColorization, lab2rgb, rgb2lab
from colddiff.snow import Snow
from colddiff.snow import SnowDiffusion as GaussianDiffusion
from .get_dataset import get_dataset

__all__ = ["GaussianDiffusion", "Trainer", "Snow", "DeColorization", "get_dataset", "rgb2lab", "lab2rgb"]
