from colddiff.decolor import UnetConvNextBlock

__all__ = ["UnetConvNextBlock"]
