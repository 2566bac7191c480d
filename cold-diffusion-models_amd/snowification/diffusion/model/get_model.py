from colddiff.decolor import UnetConvNextBlock, get_model

__all__ = ["UnetConvNextBlock", "get_model"]
