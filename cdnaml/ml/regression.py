from ..models.regression import (DecisionTreeRegressionModel, DecisionTreeRegressor, GBTRegressionModel,  # noqa: F401
                                 GBTRegressor, GeneralizedLinearRegression, GeneralizedLinearRegressionModel,
                                 GeneralizedLinearRegressionSummary, GeneralizedLinearRegressionTrainingSummary,
                                 IsotonicRegression, IsotonicRegressionModel, LinearRegression,
                                 LinearRegressionModel, RandomForestRegressionModel, RandomForestRegressor)
