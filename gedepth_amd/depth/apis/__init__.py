from .inference import inference_depther, init_depther

__all__ = ['init_depther', 'inference_depther']
