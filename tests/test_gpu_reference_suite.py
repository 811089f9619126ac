"""The scorer and loss contracts that code written against the reference's interface relies on, checked on the product on the GPU.

tests/reference_suite/contract_checks.py -- this project's own checks: result shapes, list and zero-padded tensor inputs scoring alike,
scores against a float64 restatement, the known answers of the loss classes and of the ColbertModule helpers -- runs in a subprocess
whose `colpali_engine` package is tests/reference_suite/stub (scorers and loss classes = colpali_amd's), so the product is called the
way such code calls it.  See tests/reference_suite/README.md."""
import pytest

from tests.helpers import run_contract_checks

pytestmark = pytest.mark.gpu


def test_reference_scorer_tests_pass_on_the_product():
    out = run_contract_checks("scorer", "cuda:0")
    assert "2 passed" in out, out


def test_reference_loss_class_tests_pass_on_the_product():
    out = run_contract_checks("losses", "cuda:0")
    assert "7 passed" in out, out          # ColbertLoss 2, PairwiseCE 1, NegativeCE 2, PairwiseNegativeCE 2


def test_reference_helper_tests_pass_on_the_product():
    out = run_contract_checks("helpers", "cpu")
    assert "6 passed" in out, out
