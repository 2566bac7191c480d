from colddiff.decolor import DeColorization, ForwardProcessBase

__all__ = ["DeColorization", "ForwardProcessBase"]
