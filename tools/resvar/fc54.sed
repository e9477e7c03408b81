fb_plan.h	s#constexpr int FR = 16, FC = 56;#constexpr int FR = 16, FC = 54;#
