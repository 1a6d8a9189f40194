#pragma once
#include "../juce_stub.h"
