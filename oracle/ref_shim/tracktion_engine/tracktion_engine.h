#pragma once
namespace tracktion_engine {}
