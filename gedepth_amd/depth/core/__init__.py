from .evaluation import (ErrorMaps, PriorSweep, StrataSpec, calculate, eval_metrics, metrics, metrics_from_sums, pre_eval_to_metrics,
                         strata_table)
from .utils import add_prefix

__all__ = ['ErrorMaps', 'PriorSweep', 'StrataSpec', 'calculate', 'eval_metrics', 'metrics', 'metrics_from_sums', 'pre_eval_to_metrics',
           'strata_table', 'add_prefix']
