"""reference sbgm/cli/launch_evaluation.py:4-9"""
from ..evaluate_sbgm.evaluation_main import evaluation_main


def run(cfg):
    return evaluation_main(cfg)
