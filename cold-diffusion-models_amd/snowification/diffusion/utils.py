from colddiff.decolor import lab2rgb, rgb2lab

__all__ = ["rgb2lab", "lab2rgb"]
