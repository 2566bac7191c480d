from colddiff.decolor import DecolorDiffusion as GaussianDiffusion
from colddiff.decolor import DecolorTrainer as Trainer
from colddiff.decolor import DeColorization, lab2rgb, rgb2lab
from .get_dataset import get_dataset

__all__ = ["GaussianDiffusion", "Trainer", "DeColorization", "get_dataset", "rgb2lab", "lab2rgb"]
