from colddiff.decolor import DeColorization, ForwardProcessBase
from colddiff.snow import Snow, clipped_zoom

__all__ = ["Snow", "DeColorization", "ForwardProcessBase", "clipped_zoom"]
