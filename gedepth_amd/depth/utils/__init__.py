from .color_depth import colorize
from .position_encoding import SinePositionalEncoding

__all__ = ['SinePositionalEncoding', 'colorize']
