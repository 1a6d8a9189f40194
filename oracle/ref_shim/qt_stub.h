/* Stand-in for the Qt headers the reference's SamplerSynthVoice.cpp reaches (QObject, QDebug, QCoreApplication, QList,
 * QVariant, QAbstractListModel).  Written from what the compiler asks for: a polymorphic base class, empty meta-object
 * macros, the integer typedefs, and incomplete types for everything that only appears in declarations.  No behaviour. */
#pragma once

typedef long long qint64;
typedef unsigned long long quint64;

class QString;
class QByteArray;
class QModelIndex;
template <typename T> class QList;
template <typename K, typename V> class QHash;
class QVariant {};
typedef QList<QVariant> QVariantList;

#define Q_OBJECT
#define Q_PROPERTY(...)
#define Q_SIGNAL
#define Q_SLOT
#define Q_INVOKABLE
#define Q_EMIT

class QObject {
public:
    explicit QObject(QObject * = nullptr) {}
    virtual ~QObject() {}
};
template <typename T> inline T qobject_cast(QObject *object) { return static_cast<T>(object); }

#define qApp (static_cast<QObject *>(nullptr))

namespace Qt { enum ItemDataRole { UserRole = 0x0100 }; }

class QAbstractListModel : public QObject {
public:
    explicit QAbstractListModel(QObject *parent = nullptr) : QObject(parent) {}
    virtual QHash<int, QByteArray> roleNames() const = 0;
    virtual int rowCount(const QModelIndex &parent) const = 0;
    virtual QVariant data(const QModelIndex &index, int role) const = 0;
};
