from ..models.regression import (AFTSurvivalRegression, AFTSurvivalRegressionModel,  # noqa: F401
                                 DecisionTreeRegressionModel, DecisionTreeRegressor, FMRegressionModel,
                                 FMRegressor, GBTRegressionModel,
                                 GBTRegressor, GeneralizedLinearRegression, GeneralizedLinearRegressionModel,
                                 GeneralizedLinearRegressionSummary, GeneralizedLinearRegressionTrainingSummary,
                                 IsotonicRegression, IsotonicRegressionModel, LinearRegression,
                                 LinearRegressionModel, RandomForestRegressionModel, RandomForestRegressor)
